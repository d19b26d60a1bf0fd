"""numpy statement of averagedParticleLevelset / improvedParticleLevelset (reference: source/plugin/flip.cpp:365-581,
util/matrixbase.h:184-221, util/vectorbase.h:385-389), the seeded input generators of the fixture tests/golden/partls.npz
(which stores the reference's outputs only) and the recorded FLIP loop in the package's API.

Grids are [z][y][x] arrays (2-D: one plane), particles [n][3].  Every fp32 operation is a numpy float32 operation or a Python
float rounded through float32 at once (innocuous for + - * / sqrt); the four fp64 transcendentals of the eigenvalue routine go
through Python's math module, i.e. the C library the reference was compiled against."""
import math

import numpy as np

f32 = np.float32
PDELETE = 1 << 10
EPS = f32(1e-6)


def r32(x):
    return float(f32(x))


def radius_of(dims, radiusFactor):
    """0.5 * calculateRadiusFactor, flip.cpp:198-200, 483: -> (radius, r, rZ, sradiusInv)"""
    is3d = dims[2] > 1
    rf = f32((math.sqrt(3.) if is3d else math.sqrt(2.)) * (float(f32(radiusFactor)) + .01))
    radius = f32(0.5 * float(rf))
    r = int(radius) + 1
    return radius, r, (r if is3d else 0), f32(1. / (4. * float(radius) * float(radius)))


def particle_index(dims, pos, pflag):
    """gridParticleIndex, flip.cpp:273-320: (first slot per cell [n], particles per cell [n], indexSys)"""
    sx, sy, sz = dims
    pos = np.asarray(pos, f32).reshape(-1, 3)
    c = pos.astype(np.int32)         # toVec3i truncates
    ok = ((np.asarray(pflag) & PDELETE) == 0) & (c[:, 0] >= 0) & (c[:, 1] >= 0) & (c[:, 2] >= 0) & (c[:, 0] < sx) & (c[:, 1] < sy) & (c[:, 2] < sz)
    ids = np.nonzero(ok)[0]
    key = c[ids, 0].astype(np.int64) + sx * (c[ids, 1].astype(np.int64) + sy * c[ids, 2].astype(np.int64))
    order = np.argsort(key, kind="stable")
    isys = ids[order].astype(np.int32)
    cnt = np.bincount(key, minlength=sx * sy * sz).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    return start, cnt, isys


def _norm(gx, gy, gz, px, py, pz):
    """fabs(norm(g - p)) on float32 arrays"""
    dx, dy, dz = gx - px, gy - py, gz - pz
    l = dx * dx + dy * dy + dz * dz
    eps2 = EPS * EPS
    out = np.sqrt(l)
    out = np.where(np.abs(l.astype(np.float64) - 1.) < float(eps2), f32(1), out)
    return np.where(l <= eps2, f32(0), out).astype(f32)


def gather(dims, pos, pflag, radiusFactor, ptype=None, exclude=0):
    """ComputeAveragedLevelsetWeight, flip.cpp:366-421, on every cell: (phi, pAcc [z][y][x][3], rAcc, info); the sums run in the
    reference's order zj, yj, xj, slot, vectorised over the cells"""
    sx, sy, sz = dims
    n = sx * sy * sz
    radius, r, rZ, sinv = radius_of(dims, radiusFactor)
    pos = np.asarray(pos, f32).reshape(-1, 3)
    start, cnt, isys = particle_index(dims, pos, pflag)
    kk, jj, ii = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    kk, jj, ii = kk.ravel(), jj.ravel(), ii.ravel()
    gx, gy, gz = ii.astype(f32) + f32(0.5), jj.astype(f32) + f32(0.5), kk.astype(f32) + f32(0.5)
    wacc, racc = np.zeros(n, f32), np.zeros(n, f32)
    pacc = np.zeros((n, 3), f32)
    skip = np.zeros(len(pos), bool) if ptype is None else (np.asarray(ptype) & exclude) != 0
    for dz in range(-rZ, rZ + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                x, y, z = ii + dx, jj + dy, kk + dz
                inb = (x >= 0) & (x < sx) & (y >= 0) & (y < sy) & (z >= 0) & (z < sz)
                nb = np.where(inb, x + sx * (y + sy * z), 0)
                c = np.where(inb, cnt[nb], 0)
                for slot in range(int(c.max()) if n else 0):
                    cells = np.nonzero(c > slot)[0]
                    p = isys[start[nb[cells]] + slot]
                    keep = ~skip[p]
                    cells, p = cells[keep], p[keep]
                    px, py, pz = pos[p, 0], pos[p, 1], pos[p, 2]
                    ex, ey, ez = gx[cells] - px, gy[cells] - py, gz[cells] - pz
                    s = (ex * ex + ey * ey + ez * ez) * sinv
                    w = np.maximum(0., 1. - s.astype(np.float64)).astype(f32)
                    wacc[cells] += w
                    racc[cells] += radius * w
                    pacc[cells, 0] += px * w
                    pacc[cells, 1] += py * w
                    pacc[cells, 2] += pz * w
    hit = wacc > EPS
    wd = np.where(hit, wacc, f32(1))
    rA = np.where(hit, racc / wd, f32(0)).astype(f32)
    pA = np.where(hit[:, None], pacc / wd[:, None], f32(0)).astype(f32)
    phi = np.where(hit, _norm(gx, gy, gz, pA[:, 0], pA[:, 1], pA[:, 2]) - rA, radius).astype(f32)
    info = dict(tiny=int(((wacc > 0) & ~hit).sum()), hit=int(hit.sum()), max_per_cell=int(cnt.max()) if n else 0, indexed=len(isys))
    shape = (sz, sy, sx)
    return phi.reshape(shape), pA.reshape(shape + (3,)), rA.reshape(shape), info


def max_eigenvalue(v, counts=None):
    """max(max(e0, e1), e2) of Matrix3x3f::eigenvalues, util/matrixbase.h:184-221; v: nine fp32 values v00 .. v22 as floats"""
    v00, v01, v02, v10, v11, v12, v20, v21, v22 = v
    R = r32
    b = R(R(-v00 - v11) - v22)
    c = R(R(R(R(R(v00 * R(v11 + v22)) + R(v11 * v22)) - R(v12 * v21)) - R(v01 * v10)) - R(v02 * v20))
    d = R(R(R(-v00 * R(R(v11 * v22) - R(v12 * v21))) - R(v20 * R(R(v01 * v12) - R(v11 * v02)))) - R(v10 * R(R(v02 * v21) - R(v22 * v01))))
    f = R((3.0 * c - R(b * b)) / 3.0)
    g = R((2.0 * b * b * b - 9.0 * b * c + 27.0 * d) / 27.0)
    h = R(R(g * g) / 4.0 + R(R(f * f) * f) / 27.0)
    e1 = e2 = 0.0
    if h > 0:
        branch = "pos"
        sh = R(math.sqrt(h))                       # std::sqrt of a Real: the fp32 root
        r_ = R(-g / 2.0 + sh)
        sign = 1.0
        if r_ < 0:
            r_, sign = -r_, -1.0
        s = R(sign * math.pow(r_, 1.0 / 3.0))
        t = R(-g / 2.0 - sh)
        sign = 1.0
        if t < 0:
            t, sign = -t, -1.0
        u = R(sign * math.pow(t, 1.0 / 3.0))
        e0 = R(R(s + u) - b / 3.0)
    elif h == 0:
        branch = "zero"
        e0 = R(-1.0 * 1.0 * math.pow(abs(d), 1.0 / 3.0))
    else:
        branch = "neg"
        i = R(math.sqrt(R(g * g) / 4.0 - h))
        j = R(math.pow(i, 1.0 / 3.0))
        arg = -g / (2.0 * i) if i != 0 else float("nan")
        k = R(math.acos(arg)) if -1.0 <= arg <= 1.0 else float("nan")      # acos outside [-1, 1]: NaN, as in C
        l = -j
        m = R(math.cos(k / 3.0)) if k == k else k
        nn = R(math.sqrt(3.0) * math.sin(k / 3.0)) if k == k else k
        p = R(-b / 3.0)
        e0 = R(2e0 * j * m + p)
        e1 = R(R(l * R(m + nn)) + p)
        e2 = R(R(l * R(m - nn)) + p)
    if counts is not None:
        counts[branch] = counts.get(branch, 0) + 1
    a = e1 if e0 < e1 else e0          # std::max(a, b) = (a < b) ? b : a
    return e2 if a < e2 else a


def jacobian(P, k, j, i):
    """central differences of pAcc ([z][y][x][3]) at an interior cell, v00 .. v22; in 2-D the z stride is 0: a zero column"""
    kp, km = (k + 1, k - 1) if P.shape[0] > 1 else (k, k)
    v = []
    for comp in range(3):
        v += [r32(0.5 * r32(float(P[k, j, i + 1, comp]) - float(P[k, j, i - 1, comp]))),
              r32(0.5 * r32(float(P[k, j + 1, i, comp]) - float(P[k, j - 1, i, comp]))),
              r32(0.5 * r32(float(P[kp, j, i, comp]) - float(P[km, j, i, comp])))]
    return v


def stage_bound(pAcc, rAcc, cell, t_low, t_high, phi_ref):
    """the bound on |phi - phi_ref| of a corrected cell whose fp64 pow / acos / cos / sin rounded the other way on the device:
    rAcc * 3 / (t_high - t_low) * 4 * 2^-23 * max(1, |maxEV|) + 2^-23 * |phi_ref|"""
    k, j, i = cell
    ev = max_eigenvalue(jacobian(pAcc, k, j, i))
    ev = abs(ev) if ev == ev else 1.0
    return float(rAcc[k, j, i]) * 3.0 / (r32(t_high) - r32(t_low)) * 4 * 2.0 ** -23 * max(1.0, ev) + 2.0 ** -23 * abs(float(phi_ref))


def correct(phi, pAcc, rAcc, radius, t_low, t_high, counts=None):
    """correctLevelset, flip.cpp:502-537, on the interior; returns the new phi"""
    sz, sy, sx = phi.shape
    is3d = sz > 1
    out = phi.copy()
    t_low, t_high = r32(t_low), r32(t_high)
    P = pAcc.astype(np.float64)          # fp32 values held in Python floats below
    counts = counts if counts is not None else {}
    for key in ("pos", "zero", "neg", "corrected", "below_one", "clamp0", "clamp1", "nan"):
        counts.setdefault(key, 0)
    rad = float(radius)
    for k in (range(1, sz - 1) if is3d else [0]):
        for j in range(1, sy - 1):
            for i in range(1, sx - 1):
                ra = float(rAcc[k, j, i])
                if ra <= float(EPS):
                    continue
                ev = max_eigenvalue(jacobian(P, k, j, i), counts)
                counts["corrected"] += 1
                corr = 1.0
                if ev != ev:
                    counts["nan"] += 1
                if ev >= t_low:
                    t = r32(r32(t_high - ev) / r32(t_high - t_low))
                    corr = r32(r32(r32(r32(t * t) * t) - r32(r32(3.0 * t) * t)) + r32(3.0 * t))
                if corr < 0.0:
                    corr = 0.0
                    counts["clamp0"] += 1
                elif corr > 1.0:
                    corr = 1.0
                    counts["clamp1"] += 1
                if corr < 1.0:
                    counts["below_one"] += 1
                one = lambda a: np.array([a], f32)
                dist = float(_norm(one(i + 0.5), one(j + 0.5), one(k + 0.5), one(P[k, j, i, 0]), one(P[k, j, i, 1]), one(P[k, j, i, 2]))[0])
                x = r32(dist - r32(ra * corr))
                out[k, j, i] = f32(rad if x > rad else x)
    return out


def _stencil_sum(me, factor):
    """sum * factor on the interior (centre, +x, -x, +y, -y, +z, -z) of a [z][y][x] float32 array"""
    sz, sy, sx = me.shape
    if sz > 1:
        c = me[1:-1, 1:-1, 1:-1]
        v = c + me[1:-1, 1:-1, 2:] + me[1:-1, 1:-1, :-2] + me[1:-1, 2:, 1:-1] + me[1:-1, :-2, 1:-1]
        v = v + (me[2:, 1:-1, 1:-1] + me[:-2, 1:-1, 1:-1])
    else:
        c = me[:, 1:-1, 1:-1]
        v = c + me[:, 1:-1, 2:] + me[:, 1:-1, :-2] + me[:, 2:, 1:-1] + me[:, :-2, 1:-1]
    return (v * factor).astype(f32), c


def _interior(a):
    return a[1:-1, 1:-1, 1:-1] if a.shape[0] > 1 else a[:, 1:-1, 1:-1]


def smooth(phi, smoothen, smoothenNeg):
    """the post-processing loop of flip.cpp:487-498 / 559-580 with setBound(0.5, 0)"""
    phi = phi.copy()
    factor = f32(1. / (7. if phi.shape[0] > 1 else 5.))
    for it in range(max(smoothen, smoothenNeg)):
        tmp = np.zeros_like(phi)
        if it < smoothen:
            v, _ = _stencil_sum(phi, factor)
            _interior(tmp)[...] = v
            phi, tmp = tmp, phi
        if it < smoothenNeg:
            v, c = _stencil_sum(phi, factor)
            t = _interior(tmp)
            t[...] = np.where(v < t, v, c)
            phi, tmp = tmp, phi
    set_bound(phi, f32(0.5))
    return phi


def set_bound(a, value):
    a[:, 0, :] = value
    a[:, -1, :] = value
    a[:, :, 0] = value
    a[:, :, -1] = value
    if a.shape[0] > 1:
        a[0] = value
        a[-1] = value


def particle_levelset(dims, pos, pflag, improved, radiusFactor=1., smoothen=1, smoothenNeg=1, t_low=0.4, t_high=3.5, ptype=None, exclude=0,
                      stage=None):
    """both plugins: (phi, info); stage: a (phi, pAcc, rAcc, info) of gather() to start from"""
    phi, pA, rA, info = stage if stage is not None else gather(dims, pos, pflag, radiusFactor, ptype, exclude)
    info = dict(info)
    if improved:
        counts = {}
        phi = correct(phi, pA, rA, radius_of(dims, radiusFactor)[0], t_low, t_high, counts)
        info.update(counts)
    return smooth(phi, smoothen, smoothenNeg), info


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------------
_tiny_cache = {}


def _tiny_weight_particle(centre, radiusFactor, is3d):
    """a position whose weight at `centre` is in (0, 1e-6]: on the diagonal at the edge of the support of 2 * radius, moved by a few
    units in the last place of x and y until the fp32 weight falls into the window"""
    key = (tuple(centre), radiusFactor, is3d)
    if key in _tiny_cache:
        return _tiny_cache[key]
    radius, _, _, sinv = radius_of((4, 4, 4 if is3d else 1), radiusFactor)
    g = np.asarray(centre, f32)
    base = (g + f32(float(f32(radiusFactor)) + .01) * np.array([1, 1, 1 if is3d else 0], f32)).astype(f32)
    steps = np.arange(-48, 49)
    ulp = np.spacing(base)
    px = (base[0] + steps * ulp[0]).astype(f32)[:, None]
    if is3d:
        py, pz = (base[1] + steps * ulp[1]).astype(f32)[None, :], base[2]
    else:       # the z offset inside the one plane enters the distance as well, and its square is as fine as needed
        py, pz = base[1], (g[2] + np.linspace(0, 0.02, 4001)).astype(f32)[None, :]
    ex, ey, ez = g[0] - px, g[1] - py, g[2] - pz
    s = (ex * ex + ey * ey + ez * ez) * sinv
    w = np.maximum(0., 1. - s.astype(np.float64)).astype(f32)
    hit = np.argwhere((w > 0) & (w <= EPS))
    assert len(hit), "no position with a weight in (0, 1e-6]"
    a, b = hit[0]
    _tiny_cache[key] = np.array([px[a, 0], py[0, b], pz], f32) if is3d else np.array([px[a, 0], py, pz[0, b]], f32)
    return _tiny_cache[key]


def make_particles(dims, seed, jitter, radiusFactor=1., tiny=True, empty=False):
    """a two-per-axis lattice blob (low x, low y) over a floor layer, jittered; ten strays near the top; a particle exactly on a
    cell centre; one whose weight at a neighbouring, otherwise empty cell centre is in (0, 1e-6]; deleted and out-of-domain
    particles; and a ptype channel.  -> pos [n][3], pflag [n], ptype [n]"""
    sx, sy, sz = dims
    is3d = sz > 1
    rng = np.random.RandomState(seed)
    if empty:
        return np.zeros((0, 3), f32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    zs = np.arange(1, sz - 1) if is3d else np.array([0])
    sub = np.array([0.25, 0.75], f32)
    cells = []
    for k in zs:
        for j in range(1, sy - 1):
            for i in range(1, sx - 1):
                blob = i < sx // 2 and j < (2 * sy) // 3 and (not is3d or sz // 4 <= k < sz - sz // 4)
                if blob or j < 2:
                    cells.append((i, j, k))
    cells = np.array(cells, f32)
    offs = np.array([(a, b, c) for c in (sub if is3d else [f32(0.5)]) for b in sub for a in sub], f32)
    pos = (cells[:, None, :] + offs[None, :, :]).reshape(-1, 3).astype(f32)
    if jitter:
        jit = rng.uniform(-jitter, jitter, pos.shape).astype(f32)
        if not is3d:
            jit[:, 2] = 0
        pos = (pos + jit).astype(f32)
    lo_top, hi_top = sy - 4.5, sy - 1.2
    stray = np.stack([rng.uniform(1.2, max(sx - 8.0, 2.5), 10), rng.uniform(lo_top, hi_top, 10),
                      rng.uniform(1.2, sz - 1.2, 10) if is3d else np.full(10, 0.5)], axis=1).astype(f32)
    extra = [stray, np.array([[sx // 2 + 1.5, (2 * sy) // 3 + 0.5, (sz // 2 + 0.5) if is3d else 0.5]], f32)]     # exactly a cell centre
    if tiny:
        centre = (sx - 4 + 0.5, sy - 4 + 0.5, (sz - 4 + 0.5) if is3d else 0.5)
        extra.append(_tiny_weight_particle(centre, radiusFactor, is3d)[None, :])
    outside = np.array([[-0.5, 3.2, 0.5], [sx + 0.25, 2.0, 0.5], [2.5, sy + 1.5, 0.5], [3.5, -2.0, 0.5], [2.5, 2.5, sz + 0.5], [2.5, 2.5, -1.5]], f32)
    pos = np.concatenate([pos] + extra + [outside]).astype(f32)
    perm = rng.permutation(len(pos))        # particle order is not cell order
    pos = pos[perm]
    pflag = np.where(rng.uniform(size=len(pos)) < 0.04, PDELETE, 0).astype(np.int32)
    core = len(cells) * len(offs)
    pflag[np.nonzero(perm >= core)[0]] = 0           # the special particles stay active
    ptype = rng.choice([0, 1, 2, 4, 6], size=len(pos), p=[0.6, 0.1, 0.1, 0.1, 0.1]).astype(np.int32)
    return pos, pflag, ptype


B3, S3, B2, S2 = (16, 14, 12), (12, 10, 9), (24, 20, 1), (14, 11, 1)
EXCLUDE = 4


def _case(dims, seed, jitter, rf, improved, smooth, t=(0.4, 3.5), ptype=False, empty=False):
    return dict(dims=dims, seed=seed, jitter=jitter, radiusFactor=rf, improved=improved, smoothen=smooth[0], smoothenNeg=smooth[1],
                t_low=t[0], t_high=t[1], ptype=ptype, empty=empty)


CASES = {
    "avg/b3_r1_j05_s11": _case(B3, 1, 0.05, 1.0, False, (1, 1)),
    "avg/b3_r2_j20_s20": _case(B3, 2, 0.2, 1.5, False, (2, 0)),
    "avg/b3_r1_j05_s00_ptype": _case(B3, 1, 0.05, 1.0, False, (0, 0), ptype=True),
    "avg/s3_r3_j05_s02": _case(S3, 3, 0.05, 2.5, False, (0, 2)),
    "avg/s3_r1_j20_s13": _case(S3, 4, 0.2, 1.0, False, (1, 3)),
    "avg/b2_r1_j20_s31": _case(B2, 5, 0.2, 1.0, False, (3, 1)),
    "avg/b2_r2_j05_s00": _case(B2, 6, 0.05, 1.5, False, (0, 0)),
    "avg/s2_r2_j05_s13": _case(S2, 7, 0.05, 1.3, False, (1, 3)),
    "avg/s3_empty_s11": _case(S3, 8, 0, 1.0, False, (1, 1), empty=True),
    "avg/s2_empty_s00": _case(S2, 9, 0, 1.0, False, (0, 0), empty=True),
    "imp/b3_r1_j00_s00": _case(B3, 11, 0, 1.0, True, (0, 0)),
    "imp/b3_r1_j05_s11": _case(B3, 1, 0.05, 1.0, True, (1, 1)),
    "imp/b3_r2_j20_s20": _case(B3, 12, 0.2, 1.3, True, (2, 0)),
    "imp/b3_r1_j20_s31_t": _case(B3, 13, 0.2, 1.0, True, (3, 1), t=(0.9, 1.2)),
    "imp/b3_r1_j05_s11_ptype": _case(B3, 1, 0.05, 1.0, True, (1, 1), ptype=True),
    "imp/s3_r3_j05_s02": _case(S3, 3, 0.05, 2.5, True, (0, 2)),
    "imp/s3_r2_j05_s13_t": _case(S3, 14, 0.05, 1.5, True, (1, 3), t=(0.9, 1.2)),
    "imp/b2_r1_j00_s00": _case(B2, 15, 0, 1.0, True, (0, 0)),
    "imp/b2_r1_j20_s13": _case(B2, 5, 0.2, 1.0, True, (1, 3)),
    "imp/b2_r2_j05_s20_t": _case(B2, 6, 0.05, 1.5, True, (2, 0), t=(0.9, 1.2)),
    "imp/s2_r2_j05_s11": _case(S2, 7, 0.05, 1.3, True, (1, 1)),
    "imp/s2_empty_s11": _case(S2, 9, 0, 1.0, True, (1, 1), empty=True),
}


def case_inputs(name):
    c = CASES[name]
    tiny = c["dims"] in (B3, B2)
    pos, pflag, ptype = make_particles(c["dims"], c["seed"], c["jitter"], c["radiusFactor"], tiny=tiny, empty=c["empty"])
    return dict(pos=pos, pflag=pflag, ptype=ptype if c["ptype"] else None, exclude=EXCLUDE if c["ptype"] else 0)


def case_kwargs(name):
    c = CASES[name]
    kw = dict(radiusFactor=c["radiusFactor"], smoothen=c["smoothen"], smoothenNeg=c["smoothenNeg"])
    if c["improved"]:
        kw.update(t_low=c["t_low"], t_high=c["t_high"])
    return kw


_model_cache = {}


def model_case(name):
    """(phi, stage phi [the same call with smoothen = smoothenNeg = 0], info, gather results) of a fixture case; computed once per
    process and read-only"""
    if name not in _model_cache:
        c, I = CASES[name], case_inputs(name)
        st = gather(c["dims"], I["pos"], I["pflag"], c["radiusFactor"], I["ptype"], I["exclude"])
        kw = case_kwargs(name)
        phi, info = particle_levelset(c["dims"], I["pos"], I["pflag"], c["improved"], ptype=I["ptype"], exclude=I["exclude"], stage=st, **kw)
        kw.update(smoothen=0, smoothenNeg=0)
        stage, _ = particle_levelset(c["dims"], I["pos"], I["pflag"], c["improved"], ptype=I["ptype"], exclude=I["exclude"], stage=st, **kw)
        for a in (phi, stage) + st[:3]:
            a.setflags(write=False)
        _model_cache[name] = (phi, stage, info, st)
    return _model_cache[name]


def random_inputs(dims, seed, n, crowded=6):
    """n particles: most in a slab of the domain, `crowded` cells with 40 or more each, long empty stretches elsewhere"""
    sx, sy, sz = dims
    is3d = sz > 1
    rng = np.random.RandomState(seed)
    hi = np.array([sx, sy * 0.4, sz if is3d else 1], np.float64)
    pos = rng.uniform(0.0, 1.0, (n, 3)) * hi
    for c in range(crowded):
        cell = np.array([rng.randint(1, sx - 1), rng.randint(int(sy * 0.6), sy - 1), rng.randint(1, sz - 1) if is3d else 0])
        m = 40 + c * 5
        pos[c * 64:c * 64 + m] = cell + rng.uniform(0.0, 1.0, (m, 3))
    if not is3d:
        pos[:, 2] = 0.5
    pos = pos.astype(f32)
    pos[rng.randint(0, n, 20)] += f32(sx + 3)          # out of the domain
    pflag = np.where(rng.uniform(size=n) < 0.05, PDELETE, 0).astype(np.int32)
    ptype = rng.choice([0, 1, 2, 4], size=n).astype(np.int32)
    return dict(pos=pos, pflag=pflag, ptype=ptype, exclude=EXCLUDE)


# ---------------------------------------------------------------------------------------------------------------------------------
# the recorded loop: scenes/flip02_surface.py's step (dam break) without adjustNumber and mesh output, with one of the two level
# sets in the place of unionParticleLevelset
# ---------------------------------------------------------------------------------------------------------------------------------
LOOPS = {"loop_improved": dict(improved=True), "loop_averaged": dict(improved=False)}
LOOP_RES, LOOP_STEPS, LOOP_EVERY = 32, 10, 7


def flip_loop(m, improved, res=LOOP_RES, steps=LOOP_STEPS, after_levelset=None):
    """returns the CG iterations per step and phi, vel and every LOOP_EVERY-th particle at the end; after_levelset(t, phi, pp, pindex,
    gpi, flags) is called right after the level-set plugin"""
    gs = m.vec3(res, res, res)
    s = m.Solver(name="main", gridSize=gs, dim=3)
    s.timestep = 0.8
    flags, phi, vel, velOld = s.create(m.FlagGrid), s.create(m.LevelsetGrid), s.create(m.MACGrid), s.create(m.MACGrid)
    pressure, tmpVec3 = s.create(m.RealGrid), s.create(m.VecGrid)
    pp = s.create(m.BasicParticleSystem)
    pVel = pp.create(m.PdataVec3)
    pindex, gpi = s.create(m.ParticleIndexSystem), s.create(m.IntGrid)
    flags.initDomain(boundaryWidth=1)
    fluidbox = m.Box(parent=s, p0=gs * m.vec3(0, 0, 0), p1=gs * m.vec3(0.4, 0.6, 1))
    phiInit = fluidbox.computeLevelset()
    flags.updateFromLevelset(phiInit)
    m.sampleLevelsetWithParticles(phi=phiInit, flags=flags, parts=pp, discretization=2, randomness=0.05)
    iters = []
    for t in range(steps):
        pp.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4, deleteInObstacle=False)
        m.mapPartsToMAC(vel=vel, flags=flags, velOld=velOld, parts=pp, partVel=pVel, weight=tmpVec3)
        m.extrapolateMACFromWeight(vel=vel, distance=2, weight=tmpVec3)
        m.markFluidCells(parts=pp, flags=flags)
        m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
        if improved:
            m.improvedParticleLevelset(pp, pindex, flags, gpi, phi, 1.0, 1, 1)
        else:
            m.averagedParticleLevelset(pp, pindex, flags, gpi, phi, 1.0, 1, 1)
        if after_levelset:
            after_levelset(t, phi, pp, pindex, gpi, flags)
        m.resetOutflow(flags=flags, parts=pp, index=gpi, indexSys=pindex)
        m.extrapolateLsSimple(phi=phi, distance=4, inside=True)
        m.addGravity(flags=flags, vel=vel, gravity=(0, -0.001, 0))
        m.setWallBcs(flags=flags, vel=vel)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure, phi=phi)
        iters.append(int(m.lastCgStats()["iterations"]))
        m.setWallBcs(flags=flags, vel=vel)
        m.extrapolateMACSimple(flags=flags, vel=vel)
        m.flipVelocityUpdate(vel=vel, velOld=velOld, flags=flags, parts=pp, partVel=pVel, flipRatio=0.97)
        s.step()
    return dict(iters=np.array(iters, np.int64), phi=phi.to_numpy(), vel=vel.to_numpy(), pos=pp.get_positions()[::LOOP_EVERY],
                np=np.array([pp.pySize()], np.int64))
