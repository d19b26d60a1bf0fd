"""numpy model of the turbulence model (plugin/kepsilon.cpp, the diagnostics of plugin/waveletturbulence.cpp, the turbulence
particles of turbulencepart.cpp): the executable statement of the fp32 / fp64 map of DESIGN.md section 14, the seeded input
generators of the fixture tests/golden/turbulence.npz (inputs are regenerated here, never stored; tools/record_turbulence.py records
the reference's outputs), and, at the end, the same cases and the loop of tools/tests/test_2025_turb.py through the package.

The model follows the reference pass by pass -- GetCentered into a grid, FillInBoundary as the serial in-place sweep it is, the
clamp pass, the production pass; LaplaceOp into the one `res` grid that lives through all five fields of the gradient diffusion --
where the library runs one fused kernel per plugin.  Agreement of the two is therefore a statement about the fusion as well.

Scalar grids are float32 [sz][sy][sx], vector grids float32 [sz][sy][sx][3].  Every function returns new arrays.  `cnt`, where
given, counts how many cells took each branch.
"""
import hashlib

import numpy as np

f32, f64 = np.float32, np.float64

# kepsilon.cpp:24-35, `const Real c = <double literal>`
keCmu, keC1, keC2, keS1, keS2 = f32(0.09), f32(1.44), f32(1.92), f32(1.0), f32(1.3)
keU0, keImin, keImax, keNuMin, keNuMax = f32(1.0), f32(2e-3), f32(1.0), f32(1e-3), f32(5.0)
TypeFluid, TypeObstacle, TypeEmpty = 1, 2, 4


def _k_limit(x):
    """1.5*square(keU0)*square(x): (double * Real) * Real, rounded into a const Real"""
    x = f32(x)
    return f32(1.5 * f64(keU0 * keU0) * f64(x * x))


minK, maxK = _k_limit(keImin), _k_limit(keImax)


def _bump(cnt, key, mask):
    if cnt is not None:
        cnt[key] = cnt.get(key, 0) + int(np.count_nonzero(mask))


def _half(x):
    """0.5 * x with the double literal, stored to a Real: an exact halving"""
    return (0.5 * x.astype(f64)).astype(f32)


def is3d(a):
    return a.shape[0] > 1


def interior(shape):
    """the cells of KERNEL(bnd = 1) as a tuple of slices"""
    z = slice(1, shape[0] - 1) if shape[0] > 1 else slice(0, 1)
    return (z, slice(1, shape[1] - 1), slice(1, shape[2] - 1))


def _sh(I, dz, dy, dx):
    """the interior slices shifted by (dx, dy, dz)"""
    def mv(s, d):
        return slice(s.start + d, s.stop + d)
    return (mv(I[0], dz), mv(I[1], dy), mv(I[2], dx))


def interior_mask(shape):
    m = np.zeros(shape, bool)
    m[interior(shape)] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# commonkernels.h
# ---------------------------------------------------------------------------------------------------------------------------------
def get_centered(vel):
    """GetCentered :126-131 into a cleared grid: v = 0.5 * (vel + Vec3(vel(i+1).x, vel(j+1).y, 0)); 3-D: v[2] += 0.5 * vel(k+1).z, a
    double sum rounded once; 2-D: v[2] = 0"""
    sh = vel.shape[:3]
    vc = np.zeros(vel.shape, f32)
    I = interior(sh)
    vc[I + (0,)] = _half(vel[I + (0,)] + vel[_sh(I, 0, 0, 1) + (0,)])
    vc[I + (1,)] = _half(vel[I + (1,)] + vel[_sh(I, 0, 1, 0) + (1,)])
    if sh[0] > 1:
        vz = _half(vel[I + (2,)] + f32(0))
        vc[I + (2,)] = (vz.astype(f64) + 0.5 * vel[_sh(I, 1, 0, 0) + (2,)].astype(f64)).astype(f32)
    return vc


def fill_in_boundary(g):
    """FillInBoundary :142-149 as it runs with one thread: every cell in k, j, i order, the six copies in the order written, in
    place.  Face cells end as the copy of their interior neighbour whatever the order; edge and corner cells depend on it."""
    g = g.copy()
    sz, sy, sx = g.shape[:3]
    kk, jj, ii = np.nonzero(~interior_mask_full(g.shape[:3]))
    for k, j, i in zip(kk, jj, ii):          # np.nonzero is C order: k outer, i inner
        if i == 0: g[k, j, i] = g[k, j, i + 1]
        if j == 0: g[k, j, i] = g[k, j + 1, i]
        if k == 0 and sz > 1: g[k, j, i] = g[k + 1, j, i]
        if i == sx - 1: g[k, j, i] = g[k, j, i - 1]
        if j == sy - 1: g[k, j, i] = g[k, j - 1, i]
        if k == sz - 1 and sz > 1: g[k, j, i] = g[k - 1, j, i]
    return g


def interior_mask_full(shape):
    """interior in all three directions (FillInBoundary is only used in 3-D)"""
    m = np.zeros(shape, bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m


def laplace_into(res, g):
    """LaplaceOp :75-80 writes the interior of res: each line `a - 2.0 * g + b` in double, the first stored to fp32, the others
    added with `+=` (one double sum rounded once each)"""
    I = interior(g.shape)
    d = lambda a: a.astype(f64)
    c = d(g[I])
    r = ((d(g[_sh(I, 0, 0, 1)]) - 2.0 * c) + d(g[_sh(I, 0, 0, -1)])).astype(f32)
    r = (d(r) + ((d(g[_sh(I, 0, 1, 0)]) - 2.0 * c) + d(g[_sh(I, 0, -1, 0)]))).astype(f32)
    if is3d(g):
        r = (d(r) + ((d(g[_sh(I, 1, 0, 0)]) - 2.0 * c) + d(g[_sh(I, -1, 0, 0)]))).astype(f32)
    res[I] = r


def curl_op(g, dst):
    """CurlOp :38-47 writes the interior of dst"""
    I = interior(g.shape[:3])
    P = lambda dz, dy, dx, c: g[_sh(I, dz, dy, dx) + (c,)]
    v = np.zeros(g[I].shape, f32)
    v[..., 2] = _half((P(0, 0, 1, 1) - P(0, 0, -1, 1)) - (P(0, 1, 0, 0) - P(0, -1, 0, 0)))
    if g.shape[0] > 1:
        v[..., 0] = _half((P(0, 1, 0, 2) - P(0, -1, 0, 2)) - (P(1, 0, 0, 1) - P(-1, 0, 0, 1)))
        v[..., 1] = _half((P(1, 0, 0, 0) - P(-1, 0, 0, 0)) - (P(0, 0, 1, 2) - P(0, 0, -1, 2)))
    dst[I] = v


def grid_norm(v):
    """GridNorm :116-118 with norm() of vectorbase.h:384-389"""
    with np.errstate(all="ignore"):
        l = ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]).astype(f32) + v[..., 2] * v[..., 2]).astype(f32)
        eps2 = f32(1e-6) * f32(1e-6)
        r = np.where(np.abs(l.astype(f64) - 1.0) < f64(eps2), f32(1), np.sqrt(l)).astype(f32)
        return np.where(l <= eps2, f32(0), r).astype(f32)


def _strain_sq(vel, vc, strain_mag_form):
    """S^2 on the interior, KnComputeProduction :63-71 / KnComputeStrainRateMag :216-229"""
    I = interior(vel.shape[:3])
    three = vel.shape[0] > 1
    dx = vel[_sh(I, 0, 0, 1) + (0,)] - vel[I + (0,)]
    dy = vel[_sh(I, 0, 1, 0) + (1,)] - vel[I + (1,)]
    if not three:
        dz = np.zeros(dx.shape, f32)
    elif strain_mag_form:
        dz = ((f32(0) - vel[I + (2,)]) + vel[_sh(I, 1, 0, 0) + (2,)]).astype(f32)
    else:
        dz = vel[_sh(I, 1, 0, 0) + (2,)] - vel[I + (2,)]
    ux = _half(vc[_sh(I, 0, 0, 1)] - vc[_sh(I, 0, 0, -1)])
    uy = _half(vc[_sh(I, 0, 1, 0)] - vc[_sh(I, 0, -1, 0)])
    uz = _half(vc[_sh(I, 1, 0, 0)] - vc[_sh(I, -1, 0, 0)]) if three else np.zeros(ux.shape, f32)
    S12, S13, S23 = _half(ux[..., 1] + uy[..., 0]), _half(ux[..., 2] + uz[..., 0]), _half(uy[..., 2] + uz[..., 1])
    diag = ((dx * dx + dy * dy).astype(f32) + dz * dz).astype(f32)
    d = lambda a: a.astype(f64)
    return (((d(diag) + 2.0 * d(S12 * S12)) + 2.0 * d(S13 * S13)) + 2.0 * d(S23 * S23)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# kepsilon.cpp
# ---------------------------------------------------------------------------------------------------------------------------------
def turbulence_clamp(k, eps, cnt=None):
    """KnTurbulenceClamp :38-50: both nu limits from the clamped k and the unclamped eps"""
    with np.errstate(all="ignore"):
        ke = np.where(k < minK, minK, np.where(k > maxK, maxK, k)).astype(f32)
        c = (keCmu * (ke * ke).astype(f32)).astype(f32)
        nu = (c / eps).astype(f32)
        e = np.where(nu > keNuMax, (c / keNuMax).astype(f32), eps)
        e = np.where(nu < keNuMin, (c / keNuMin).astype(f32), e).astype(f32)
    _bump(cnt, "k_low", k < minK)
    _bump(cnt, "k_high", k > maxK)
    _bump(cnt, "nu_high", nu > keNuMax)
    _bump(cnt, "nu_low", nu < keNuMin)
    return ke, e


def production(vel, k, eps, prod, nuT, strain=None, pscale=1.0, cnt=None):
    """KEpsilonComputeProduction :86-99 -> (k, eps, prod, nuT, strain)"""
    assert is3d(k), "KEpsilonComputeProduction: 3-D solvers only"
    vc = fill_in_boundary(get_centered(vel))
    k, eps = turbulence_clamp(k, eps, cnt)
    prod, nuT = prod.copy(), nuT.copy()
    strain = None if strain is None else strain.copy()
    I = interior(k.shape)
    with np.errstate(all="ignore"):
        e, ke = eps[I], k[I]
        pos = e > 0
        nu = ((keCmu * (ke * ke).astype(f32)).astype(f32) / e).astype(f32)
        S2 = _strain_sq(vel, vc, False)
        P = (((2.0 * nu.astype(f64)) * S2.astype(f64)) * f64(f32(pscale))).astype(f32)
        prod[I] = np.where(pos, P, f32(0))
        nuT[I] = np.where(pos, nu, f32(0))
        if strain is not None:
            strain[I] = np.where(pos, np.sqrt(S2), f32(0))
    _bump(cnt, "eps_nonpositive", e <= 0)
    _bump(cnt, "eps_nan", np.isnan(e))
    _bump(cnt, "eps_positive", pos)
    _bump(cnt, "strain_none" if strain is None else "strain_given", 1)
    return k, eps, prod, nuT, strain


def sources(k, eps, prod, dt, cnt=None):
    """KEpsilonSources :102-126 -> (k, eps)"""
    dt = f32(dt)
    with np.errstate(all="ignore"):
        ke = np.where(k <= 0, f32(1e-3), k).astype(f32)
        newK = (ke + (dt * (prod - eps)).astype(f32)).astype(f32)
        newEps = (eps + ((dt * ((prod * keC1).astype(f32) - (eps * keC2).astype(f32)).astype(f32)).astype(f32) * (eps / ke).astype(f32)).astype(f32)).astype(f32)
        _bump(cnt, "ke_nonpositive", k <= 0)
        _bump(cnt, "newEps_nonpositive", newEps <= 0)
        newEps = np.where(newEps <= 0, f32(1e-4), newEps).astype(f32)
    return turbulence_clamp(newK, newEps, cnt)


def bcs(flags, k, eps, intensity, nu, fillArea):
    """KEpsilonBcs :129-140 -> (k, eps)"""
    vk = _k_limit(intensity)
    ve = f32(f32(keCmu * f32(vk * vk)) / f32(nu))
    m = np.ones(k.shape, bool) if fillArea else (flags & TypeObstacle) != 0
    return np.where(m, vk, k).astype(f32), np.where(m, ve, eps).astype(f32)


def gradient_diffusion(k, eps, nuT, dt, sigmaU=4.0, vel=None):
    """KEpsilonGradientDiffusion :157-179 -> (k, eps, vel): one `res` grid, cleared once, goes through all fields"""
    dt = f32(dt)
    res = np.zeros(k.shape, f32)

    def apply(g, sigma):
        with np.errstate(all="ignore"):
            laplace_into(res, g)
            res[...] = res * nuT
            res[...] = res * f32(dt / f32(sigma))
            return (g + res).astype(f32)

    k = apply(k, keS1)
    eps = apply(eps, keS2)
    if vel is not None:
        vel = vel.copy()
        for c in range(3):
            vel[..., c] = apply(np.ascontiguousarray(vel[..., c]), sigmaU)
    return k, eps, vel


# ---------------------------------------------------------------------------------------------------------------------------------
# waveletturbulence.cpp
# ---------------------------------------------------------------------------------------------------------------------------------
def strain_rate_mag(vel, mag):
    """computeStrainRateMag :212-236 (no FillInBoundary: the border of the centred grid is 0)"""
    mag = mag.copy()
    mag[interior(mag.shape)] = _strain_sq(vel, get_centered(vel), True)
    return mag


def vorticity(vel, vort, norm=None):
    """computeVorticity :204-209 -> (vorticity, norm)"""
    vort = vort.copy()
    curl_op(get_centered(vel), vort)
    return vort, (None if norm is None else grid_norm(vort))


def get_curl(vel, comp):
    """getCurl :310-316"""
    curl = np.zeros(vel.shape, f32)
    curl_op(get_centered(vel), curl)
    return np.ascontiguousarray(curl[..., comp])


# ---------------------------------------------------------------------------------------------------------------------------------
# the fixture: cases, seeded inputs, and how large arrays are kept
# ---------------------------------------------------------------------------------------------------------------------------------
FULL_LIMIT = 4096      # arrays with more elements are kept in the fixture as the SHA-256 of their bytes (the file stays under 1 MB)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def put(out, key, a):
    """recorder side: the array itself, or its digest under key + '#sha' where it is large"""
    a = np.ascontiguousarray(a)
    if a.size <= FULL_LIMIT:
        out[key] = a
    else:
        out[key + "#sha"] = digest(a)


def same_as_fixture(golden, key, a):
    """-> None if `a` is, bit for bit, what the fixture recorded under key; else a message"""
    a = np.ascontiguousarray(a)
    if key in golden:
        w = golden[key]
        if a.shape != w.shape or a.dtype != w.dtype:
            return "%s: shape / dtype %s %s, recorded %s %s" % (key, a.shape, a.dtype, w.shape, w.dtype)
        u = "u%d" % a.dtype.itemsize
        d = a.view(u) != w.view(u)
        return None if not d.any() else "%s: %d of %d words differ, first at %s" % (key, int(d.sum()), d.size, np.argwhere(d)[0])
    if key + "#sha" in golden:
        return None if np.array_equal(digest(a), golden[key + "#sha"]) else "%s: the SHA-256 of %s differs from the recorded one" % (key, a.shape)
    return "%s: not in the fixture" % key


DIMS = {"g7": (7, 5, 4), "g6": (6, 6, 6), "g33": (33, 31, 29), "g2d": (12, 9, 1)}


def shape_of(dims):
    return (dims[2], dims[1], dims[0])


def _seed(name, what):
    return int.from_bytes(hashlib.sha256(("%s/%s" % (name, what)).encode()).digest()[:4], "little")


def rand_vel(name, scale=1.0):
    sh = shape_of(DIMS[name])
    v = (np.random.RandomState(_seed(name, "vel")).uniform(-1, 1, sh + (3,)) * scale).astype(f32)
    if sh[0] == 1:
        v[..., 2] = 0
    return v


def ke_inputs(name, nan=False):
    """vel, k, eps, prod, nuT scaled so that every branch occurs: k below / inside / above [minK, maxK], nu above / inside / below its
    limits, eps <= 0 (zero and negative), k <= 0.  The clamp turns every eps <= 0 of a finite cell positive, so the production's
    `eps <= 0` branch is only entered beside a NaN: with nan = True (the production cases) some cells hold k = NaN over a negative eps
    (the clamp passes both through) and some eps = NaN.  No arithmetic result of a NaN is stored in those cells: k and eps keep their
    bits, prod / nuT / strain are zeros."""
    sh = shape_of(DIMS[name])
    r = np.random.RandomState(_seed(name, "ke"))
    k = (10.0 ** r.uniform(-7, 0.7, sh)).astype(f32)
    k[r.uniform(size=sh) < 0.06] *= f32(-1)
    k[r.uniform(size=sh) < 0.03] = 0
    # eps around Cmu k^2 / nu for nu across [1e-5, 1e3]
    kk = np.clip(np.abs(k), minK, maxK).astype(f64)
    eps = (0.09 * kk * kk / 10.0 ** r.uniform(-5, 3, sh)).astype(f32)
    eps[r.uniform(size=sh) < 0.05] *= f32(-1)
    eps[r.uniform(size=sh) < 0.03] = 0
    if nan:
        rn = np.random.RandomState(_seed(name, "nan"))
        m1, m2 = rn.uniform(size=sh) < 0.04, rn.uniform(size=sh) < 0.04
        k[m1], eps[m1] = np.nan, -np.abs(eps[m1]) - f32(0.5)
        eps[m2 & ~m1] = np.nan
    prod = (10.0 ** r.uniform(-4, 1, sh)).astype(f32)
    nuT = (10.0 ** r.uniform(-3, 0.5, sh)).astype(f32)
    nuT[r.uniform(size=sh) < 0.05] *= f32(-1)      # a negative viscosity on the border leaves a negative zero in `res`
    flags = np.full(sh, TypeFluid, np.int32)
    flags[r.uniform(size=sh) < 0.2] = TypeObstacle
    flags[r.uniform(size=sh) < 0.1] = TypeEmpty
    return dict(dims=DIMS[name], vel=rand_vel(name, 2.0), k=k, eps=eps, prod=prod, nuT=nuT, flags=flags)


PRODUCTION_CASES = ("g7", "g6", "g33")
SOURCES_CASES = ("g7", "g6", "g33", "g2d")
GRADDIFF_CASES = ("g7", "g33", "g2d")
DIAG_CASES = ("g7", "g33", "g2d")
PSCALE, DT, SIGMA_U = 0.75, 0.4, 3.0
BCS = dict(intensity=0.1, nu=0.05)


def prefill(name, what):
    """what the caller's output grids hold before a call (border cells must keep it); finite, so that it can be hashed and compared"""
    sh = shape_of(DIMS[name])
    return np.random.RandomState(_seed(name, "prefill/" + what)).uniform(-9, 9, sh).astype(f32)


def run_production(name, with_strain, cnt=None):
    I = ke_inputs(name, nan=True)
    st = prefill(name, "strain") if with_strain else None
    k, eps, prod, nuT, strain = production(I["vel"], I["k"], I["eps"], prefill(name, "prod"), prefill(name, "nuT"), st, PSCALE, cnt)
    r = dict(k=k, eps=eps, prod=prod, nuT=nuT)
    if with_strain:
        r["strain"] = strain
    return r


def run_sources(name, cnt=None):
    I = ke_inputs(name)
    k, eps = sources(I["k"], I["eps"], I["prod"], DT, cnt)
    return dict(k=k, eps=eps)


def run_bcs(name, fillArea):
    I = ke_inputs(name)
    k, eps = bcs(I["flags"], I["k"], I["eps"], BCS["intensity"], BCS["nu"], fillArea)
    return dict(k=k, eps=eps)


def graddiff_inputs(name):
    """fields of moderate size (the scheme is not unconditionally stable; two calls must stay finite)"""
    I = ke_inputs(name)
    r = np.random.RandomState(_seed(name, "gd"))
    sh = shape_of(DIMS[name])
    I["k"] = r.uniform(0.01, 1.0, sh).astype(f32)
    I["eps"] = r.uniform(0.01, 1.0, sh).astype(f32)
    return I


def run_graddiff(name, with_vel, calls=2):
    I = graddiff_inputs(name)
    k, eps, vel = I["k"], I["eps"], (I["vel"] if with_vel else None)
    for _ in range(calls):
        k, eps, vel = gradient_diffusion(k, eps, I["nuT"], DT, SIGMA_U, vel)
    r = dict(k=k, eps=eps)
    if with_vel:
        r["vel"] = vel
    return r


def diag_prefill_vec(name):
    sh = shape_of(DIMS[name])
    return np.random.RandomState(_seed(name, "prefill/vort")).uniform(-2, 2, sh + (3,)).astype(f32)


def run_diagnostics(name):
    vel = rand_vel(name, 2.0)
    vort, nrm = vorticity(vel, diag_prefill_vec(name), True)
    return dict(mag=strain_rate_mag(vel, prefill(name, "mag")), vort=vort, norm=nrm, curl0=get_curl(vel, 0), curl1=get_curl(vel, 1),
                curl2=get_curl(vel, 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# turbulence particles, turbulencepart.cpp
# ---------------------------------------------------------------------------------------------------------------------------------
import nbflip_model as N  # noqa: E402  (Parts with its literal compress, Grid<Real>::getInterpolated)

PDELETE = N.PDELETE
SEED = 34894231


class Stream(object):
    """util/randomstream.h: MT19937 seeded with init_genrand; getReal() = float(randInt() * (1 / 4294967295)); `cursor` reals drawn"""

    def __init__(self, cursor=0):
        self.bg = np.random.MT19937()
        self.bg._legacy_seeding(SEED)
        self.cursor = 0
        while self.cursor < cursor:
            self.vec3(min((cursor - self.cursor) // 3, 1 << 18)) if cursor - self.cursor >= 3 else self._reals(cursor - self.cursor)

    def _reals(self, n):
        self.cursor += n
        return (self.bg.random_raw(n).astype(f64) * (1.0 / 4294967295.0)).astype(f32)

    def vec3(self, m=1):
        return self._reals(3 * m).reshape(m, 3)


class State(object):
    """the statics of the reference: seed()'s stream, synthesize()'s ctime and inflow"""

    def __init__(self, cursor=0, ctime=0.0, inflow=(0, 0, 0)):
        self.stream, self.ctime, self.inflow = Stream(int(cursor)), f32(ctime), np.array(inflow, f32)

    def snapshot(self):
        """[cursor, ctime bits, inflow bits x 3] as int64"""
        return np.array([self.stream.cursor, int(np.array(self.ctime, f32).view(np.uint32))] + [int(v) for v in self.inflow.view(np.uint32)], np.int64)

    @staticmethod
    def from_snapshot(a):
        a = np.asarray(a, np.int64)
        u = a[1:].astype(np.uint32).view(f32)
        return State(int(a[0]), u[0], u[1:4])


def box_shape(center, size):
    """Box(center, size), shapes.cpp:137-152, with getCenter / getExtent of shapes.h:77-78"""
    c, s = np.array(center, f32), np.array(size, f32)
    p0, p1 = c - s, c + s
    inside = lambda p: ((p >= p0) & (p <= p1)).all(axis=1)
    return dict(center=_half(p1 + p0), extent=p1 - p0, inside=inside)


def sphere_shape(center, radius):
    """Sphere(center, radius): normSquare(pos - center) <= radius^2; extent Vec3(2.0 * radius)"""
    c, r = np.array(center, f32), f32(radius)

    def inside(p):
        d = (p - c).astype(f32)
        return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(f32) + d[:, 2] * d[:, 2]).astype(f32) <= r * r
    return dict(center=c, extent=np.full(3, f32(2.0 * f64(r)), f32), inside=inside)


def hsv2rgb(h, s, v):
    """turbulencepart.cpp:35-55 for a float32 array h"""
    s, v, one = f32(s), f32(v), f32(1)
    h6 = (h * f32(6)).astype(f32)
    i = np.trunc(h6).astype(np.int64)
    f = (h6 - i.astype(f32)).astype(f32)
    p = np.full(h.shape, v * (one - s), f32)
    q = (v * (one - (f * s).astype(f32)).astype(f32)).astype(f32)
    t = (v * (one - ((one - f).astype(f32) * s).astype(f32)).astype(f32)).astype(f32)
    vv = np.full(h.shape, v, f32)
    table = [(vv, t, p), (q, vv, p), (p, vv, t), (p, q, vv), (t, p, vv), (vv, p, q)]
    out = np.zeros(h.shape + (3,), f32)
    for case, cols in enumerate(table):
        m = np.fmod(i, 6) == case
        for c in range(3):
            out[m, c] = cols[c][m]
    return out


def new_system():
    return N.Parts(np.zeros((0, 3), f32), np.zeros(0, np.int32), [N.Channel("vec3", np.zeros((0, 3), f32)) for _ in range(3)], allow_compress=True)


def seed(P, st, shape, num, cnt=None):
    """TurbulenceParticleSystem::seed :57-68, attempt by attempt"""
    sz = shape["extent"]
    p0 = (shape["center"] - (sz * f32(0.5)).astype(f32)).astype(f32)
    pts = np.zeros((num, 3), f32)
    for q in range(num):
        while True:
            p = (st.stream.vec3() * sz + p0).astype(f32)
            if shape["inside"](p)[0]:
                break
            _bump(cnt, "seed_rejected", 1)
        pts[q] = p[0]
    z = ((pts[:, 2] - p0[2]) / sz[2]).astype(f32)
    _bump(cnt, "hue_one", z >= 1)
    col = hsv2rgb(z, 0.75, 1.0)
    P.pos = np.concatenate([P.pos, pts])
    P.flag = np.concatenate([P.flag, np.zeros(num, np.int32)])
    for ch, a in zip(P.channels, (col, pts, pts)):
        ch.data = np.concatenate([ch.data, a])
    if num > 0:
        P.chunk = P.size() // N.DELETE_PART


def evaluate_vec(tile, params, pos, t):
    """WaveletNoiseField::evaluateVec(pos, t), noisefield.h:358-385, with WNoiseVec :218-310; params: NoiseField._params()"""
    Pm = [f32(v) for v in params]
    p = [pos[:, c].astype(f32) for c in range(3)]
    p = [(p[c] * Pm[c]).astype(f32) for c in range(3)]
    p = [(p[c] + Pm[3 + c]).astype(f32) for c in range(3)]
    p = [(p[c] + Pm[6]).astype(f32) for c in range(3)]
    p = [(p[c] * Pm[7 + c]).astype(f32) for c in range(3)]
    p = [(p[c] + Pm[10 + c]).astype(f32) for c in range(3)]
    w, dw, mid = [], [], []
    one = f32(1)
    for c in range(3):
        pm = (p[c] - f32(0.5)).astype(f32)
        m = np.ceil(pm.astype(f64)).astype(np.int64)
        t_ = (m.astype(f32) - pm).astype(f32)
        u = (one - t_).astype(f32)
        w0 = ((t_ * t_).astype(f32) * f32(0.5)).astype(f32)
        w2 = ((u * u).astype(f32) * f32(0.5)).astype(f32)
        w.append((w0, ((one - w0).astype(f32) - w2).astype(f32), w2))
        dw.append(((-t_).astype(f32), ((f32(2) * t_).astype(f32) - one).astype(f32), u))
        mid.append(m)
    data = tile[t * 128 ** 3:(t + 1) * 128 ** 3]
    out = []
    for comp in range(3):
        res = np.zeros(p[0].shape, f32)
        for z in (-1, 0, 1):
            for y in (-1, 0, 1):
                for x in (-1, 0, 1):
                    a = (dw if comp == 0 else w)[0][x + 1]
                    b = (dw if comp == 1 else w)[1][y + 1]
                    c = (dw if comp == 2 else w)[2][z + 1]
                    wt = ((a * b).astype(f32) * c).astype(f32)
                    xc, yc, zc = (mid[0] + x) & 127, (mid[1] + y) & 127, (mid[2] + z) & 127
                    res = (res + (wt * data[(zc * 128 + yc) * 128 + xc]).astype(f32)).astype(f32)
        res = ((res + Pm[13]).astype(f32) * Pm[14]).astype(f32)
        if Pm[15] != 0:
            res = np.where(res < Pm[16], Pm[16], res)
            res = np.where(res > Pm[17], Pm[17], res).astype(f32)
        out.append(res)
    return np.stack(out, axis=1)


def evaluate_curl(tile, params, pos):
    d0, d1, d2 = (evaluate_vec(tile, params, pos, t) for t in range(3))
    return np.stack([d0[:, 1] - d1[:, 2], d2[:, 2] - d0[:, 0], d1[:, 0] - d2[:, 1]], axis=1).astype(f32)


def nmod1(a):
    c = np.fmod(f32(a), f32(1))
    return f32(c + f32(1)) if c < 0 else f32(c)


def in_bounds(pos, dims):
    """flags.isInBounds(pos): the truncated position inside the grid; int conversion of a NaN or a huge value gives INT_MIN"""
    with np.errstate(all="ignore"):
        ok = np.isfinite(pos).all(axis=1) & (np.abs(pos) < 2.0 ** 31).all(axis=1)
        t = np.where(ok[:, None], np.trunc(np.where(ok[:, None], pos, 0)), -1).astype(np.int64)
    lim = np.array(dims, np.int64)
    return ((t >= 0) & (t < lim)).all(axis=1)


def reset_tex(P, num, inflow):
    P.channels[1 if num == 0 else 2].data = (P.pos - inflow).astype(f32)


def synthesize(P, st, dims, kgrid, tile, params, dt, octaves=2, switchLength=10.0, L0=0.1, scale=1.0, inflowBias=(0, 0, 0), cnt=None):
    """TurbulenceParticleSystem::synthesize :112-131 and KnSynthesizeTurbulence :79-110"""
    dt, sl = f32(dt), f32(switchLength)
    st.inflow = (st.inflow + (np.array(inflowBias, f32) * dt).astype(f32)).astype(f32)
    old_alpha = f32(2) * nmod1(st.ctime / sl)
    st.ctime = f32(st.ctime + dt)
    alpha = f32(2) * nmod1(st.ctime / sl)
    if old_alpha < 1 and alpha >= 1:
        reset_tex(P, 0, st.inflow)
        _bump(cnt, "reset_tex0", 1)
    if old_alpha > alpha:
        reset_tex(P, 1, st.inflow)
        _bump(cnt, "reset_tex1", 1)
    alpha = f32(1.0)
    kmin = f32(1.5 * (0.1 * 0.1))
    _bump(cnt, "octaves_%d" % octaves, 1)
    if P.size() == 0:
        return
    m = in_bounds(P.pos, dims)
    _bump(cnt, "outside_skipped", ~m)
    _bump(cnt, "deleted_synthesized", m & ((P.flag & PDELETE) != 0))
    pos, t0, t1 = P.pos[m], P.channels[1].data[m], P.channels[2].data[m]
    k2 = (N.interp_real(kgrid, pos) - kmin).astype(f32)
    _bump(cnt, "k2_negative", k2 < 0)
    _bump(cnt, "k2_positive", k2 > 0)
    with np.errstate(invalid="ignore"):
        ks = np.where(k2 < 0, f32(0), np.sqrt(k2)).astype(f32)
    amp = (f32(scale) * ks).astype(f32)
    mult = f32(f32(1.0) / f32(L0))
    vel = np.zeros(pos.shape, f32)
    beta = f32(f32(1.0) - alpha)
    for _ in range(octaves):
        n0 = (evaluate_curl(tile, params, (t0 * mult).astype(f32)) * amp[:, None]).astype(f32)
        n1 = (evaluate_curl(tile, params, (t1 * mult).astype(f32)) * amp[:, None]).astype(f32)
        vel = (vel + ((alpha * n0).astype(f32) + (beta * n1).astype(f32)).astype(f32)).astype(f32)
        amp = (amp * f32(0.56123)).astype(f32)
        mult = f32(mult * f32(2.0))
    dx = (vel * dt).astype(f32)
    P.pos[m] = pos + dx
    P.channels[1].data[m] = t0 + dx
    P.channels[2].data[m] = t1 + dx


def delete_in_obstacle(P, flags, dims, cnt=None):
    """TurbulenceParticleSystem::deleteInObstacle :133-138.  Every position must lie inside the grid."""
    n = P.size()
    assert in_bounds(P.pos, dims).all(), "deleteInObstacle: a position outside the grid (the reference reads outside the flag grid)"
    c = np.trunc(P.pos).astype(np.int64)
    hit = (flags[c[:, 2], c[:, 1], c[:, 0]] & TypeObstacle) != 0
    P.flag = np.where(hit, P.flag | PDELETE, P.flag).astype(np.int32)
    dead = (P.flag & PDELETE) != 0
    if cnt is not None and n:
        kind = "delete_none" if not dead.any() else "delete_all" if dead.all() else "delete_some"
        _bump(cnt, kind, 1)
        _bump(cnt, "delete_last_slot", bool(dead[-1]) and not dead.all())
    P.compress_serial()


_oracle_lib = None


def oracle_advect(dims, flags, vel, P, dt):
    """ParticleSystem::advectInGrid(flags, vel, IntRK4) with its defaults (delete marks only): not restated here -- it is the
    package's existing bit-exact entry mf_advect_in_grid, taken from the CPU checker library through its C ABI"""
    global _oracle_lib
    import ctypes
    import util
    from mantaflow_amd import _lib
    if P.size() == 0:
        return
    if _oracle_lib is None:
        _oracle_lib = _lib.Library(util.build_oracle(), "cpu")
    n = P.size()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pos = np.ascontiguousarray(P.pos.T)
    flag = np.ascontiguousarray(P.flag)
    v = np.ascontiguousarray(vel.reshape(-1, 3).T)
    fl = np.ascontiguousarray(flags, np.int32)
    scratch = np.zeros(9 * n, f32)
    _oracle_lib.cdll.mf_set_slab_window(0, 0)
    _oracle_lib.call("mf_advect_in_grid", dims[0], dims[1], dims[2], ptr(fl), ptr(v), n, n, ptr(pos), ptr(flag), float(f32(dt)), 2, 1, 1, 0, None, 0,
                     ptr(scratch), None)
    P.pos, P.flag = np.ascontiguousarray(pos.T), flag


# ---- the particle cases ----
PDIMS = (20, 12, 10)
PDT = 0.5
OBSTACLE_BLOCK = ((8, 12), (4, 8), (3, 7))       # x, y, z cell ranges of the obstacle inside the domain
FREE_BOX = ((4.5, 6.0, 5.0), (1.5, 2.5, 2.0))    # centre, half size: clear of the obstacle and the walls
MIXED_BOX = ((7.5, 6.0, 5.0), (2.0, 2.0, 1.5))   # overlaps the obstacle block
INSIDE_BOX = ((10.0, 6.0, 5.0), (1.2, 1.2, 1.2))  # wholly inside it
BALL = ((5.0, 6.0, 5.0), 2.5)


def particle_grids():
    sh = shape_of(PDIMS)
    r = np.random.RandomState(_seed("parts", "grids"))
    flags = np.full(sh, TypeFluid, np.int32)
    flags[0], flags[-1], flags[:, 0], flags[:, -1], flags[:, :, 0], flags[:, :, -1] = (TypeObstacle,) * 6
    (x0, x1), (y0, y1), (z0, z1) = OBSTACLE_BLOCK
    flags[z0:z1, y0:y1, x0:x1] = TypeObstacle
    vel = r.uniform(-0.6, 0.6, sh + (3,)).astype(f32)
    k = r.uniform(0.0, 0.06, sh).astype(f32)         # kmin = 0.015 lies inside: k2 < 0 and k2 > 0 both occur
    return flags, vel, k


def _cycle(octaves, scale=0.4, switchLength=2.0, bias=(0.3, 0.0, -0.1)):
    return [("advect",), ("synth", octaves, switchLength, 0.05, scale, bias), ("delete",)]


def _scene_box(res=64):
    """the seeding box of scenes/turbulence.py: center gs * vec3(0.05, 0.43, 0.6), size gs * vec3(0.02, 0.005, 0.07), in fp32"""
    gs = np.array([res, res // 2, res // 2], f32)
    return tuple((gs * np.array([0.05, 0.43, 0.6], f32)).astype(f32)), tuple((gs * np.array([0.02, 0.005, 0.07], f32)).astype(f32))


PARTICLE_CASES = {
    # the first seeding call of scenes/turbulence.py in a fresh process (seed() touches no grid: the box lies outside this stage's)
    "scene": [("seed", "box", _scene_box(), 500)],
    "n0": [("seed", "box", MIXED_BOX, 0)] + _cycle(1),
    "n1": [("seed", "box", MIXED_BOX, 1)] + _cycle(2),
    "n63": [("seed", "box", MIXED_BOX, 63)] + _cycle(3),
    "n64": [("seed", "box", MIXED_BOX, 64)] + _cycle(1),
    "n65": [("seed", "box", MIXED_BOX, 65)] + _cycle(2),
    "n1000": [("seed", "box", MIXED_BOX, 1000)] + _cycle(3),
    "n5000": [("seed", "box", MIXED_BOX, 5000)] + _cycle(2),
    # three seeding calls on the continuing stream (a Sphere rejects the corners of its bounding box), then five steps: with
    # dt 0.5 and switchLength 2 the hat function has a period of four calls, so both resetTexCoords branches fire
    "seq": [("seed", "sphere", BALL, 200), ("seed", "box", FREE_BOX, 100), ("seed", "sphere", BALL, 150)] + _cycle(2) * 5,
    "none": [("seed", "box", FREE_BOX, 40), ("delete",)],
    "all": [("seed", "box", INSIDE_BOX, 40), ("delete",)],
    "last": [("seed", "box", FREE_BOX, 10), ("move", 9, (10.5, 6.5, 5.5)), ("delete",)],
    # a slot outside the grid is skipped by synthesize; it is back inside before deleteInObstacle (the contract)
    "outside": [("seed", "box", FREE_BOX, 5), ("move", 2, (-3.5, 4.0, 4.0)), ("synth", 1, 2.0, 0.05, 0.4, (0, 0, 0)), ("move", 2, (5.5, 4.25, 4.125)),
                ("delete",)],
}
PARTICLE_ORDER = ("scene", "n0", "n1", "n63", "n64", "n65", "n1000", "n5000", "seq", "none", "all", "last", "outside")
CHANNELS = ("pos", "color", "tex0", "tex1", "flag")


def shape_from(kind, spec):
    return box_shape(*spec) if kind == "box" else sphere_shape(*spec)


def system_state(P):
    return dict(pos=P.pos.copy(), color=P.channels[0].data.copy(), tex0=P.channels[1].data.copy(), tex1=P.channels[2].data.copy(), flag=P.flag.copy())


def run_particle_case(name, st, tile, params, cnt=None, advect=oracle_advect):
    """-> (state of the system after the last call, sizes [calls], stream cursors [calls]); st (a State) moves on"""
    flags, vel, k = particle_grids()
    P = new_system()
    sizes, cursors = [], []
    for op in PARTICLE_CASES[name]:
        if op[0] == "seed":
            seed(P, st, shape_from(op[1], op[2]), op[3], cnt)
            _bump(cnt, "seed_" + op[1], 1)
        elif op[0] == "advect":
            advect(PDIMS, flags, vel, P, PDT)
        elif op[0] == "synth":
            synthesize(P, st, PDIMS, k, tile, params, PDT, op[1], op[2], op[3], op[4], op[5], cnt)
        elif op[0] == "delete":
            delete_in_obstacle(P, flags, PDIMS, cnt)
        elif op[0] == "move":
            P.pos[op[1]] = np.array(op[2], f32)
        sizes.append(P.size())
        cursors.append(st.stream.cursor)
    return system_state(P), np.array(sizes, np.int64), np.array(cursors, np.int64)


PARTICLE_CONDITIONS = ("seed_box", "seed_sphere", "seed_rejected", "octaves_1", "octaves_2", "octaves_3", "reset_tex0", "reset_tex1", "k2_negative",
                       "k2_positive", "outside_skipped", "deleted_synthesized", "delete_none", "delete_some", "delete_all", "delete_last_slot")

# the loop of tools/tests/test_2025_turb.py at gridSize (res, res / 2, res / 2); the spheres have radius res * 0.025 = 1
LOOP = dict(res=40, steps=8, dt=1.2)


def noise_tile_and_params(dims):
    """the wavelet noise tile (3 x 128^3, bit-exact with the reference's) and the parameter block of a default NoiseField on a solver
    of these dimensions, from the package on the backend in use (the CPU checker where nothing else is set)"""
    from mantaflow_amd import _lib
    if _lib._current is None:
        import util
        _lib.use_library(util.build_oracle(), "cpu")
    import manta as m
    s = m.Solver(name="n", gridSize=m.vec3(*dims), dim=3)
    noise = s.create(m.NoiseField)
    return noise._tile.detach().cpu().numpy().copy(), np.array(list(noise._params()), f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the same cases through the package (`m` is the manta module), shared by the GPU tests and tools/turbulence_time.py
# ---------------------------------------------------------------------------------------------------------------------------------
def pkg_shape(m, s, kind, spec):
    if kind == "box":
        return m.Box(parent=s, center=m.vec3(*[float(v) for v in spec[0]]), size=m.vec3(*[float(v) for v in spec[1]]))
    return m.Sphere(parent=s, center=m.vec3(*[float(v) for v in spec[0]]), radius=float(spec[1]))


def run_particle_case_pkg(m, name, start):
    """the case through the package from the recorded start state -> (channels, sizes, cursors) like run_particle_case"""
    from mantaflow_amd import core
    st = State.from_snapshot(start)
    core._set_turbulence_particle_state(int(start[0]), st.ctime, st.inflow)
    s = m.Solver(name="p", gridSize=m.vec3(*PDIMS), dim=3)
    s.timestep = PDT
    fl, v, kk = particle_grids()
    flags, vel, k = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.RealGrid)
    flags.from_numpy(fl), vel.from_numpy(v), k.from_numpy(kk)
    turb = s.create(m.TurbulenceParticleSystem, noise=s.create(m.NoiseField))
    sizes, cursors = [], []
    for op in PARTICLE_CASES[name]:
        if op[0] == "seed":
            turb.seed(pkg_shape(m, s, op[1], op[2]), op[3])
        elif op[0] == "advect":
            turb.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4)
        elif op[0] == "synth":
            turb.synthesize(flags=flags, k=k, octaves=op[1], switchLength=op[2], L0=op[3], scale=op[4], inflowBias=m.vec3(*op[5]))
        elif op[0] == "delete":
            turb.deleteInObstacle(flags)
        elif op[0] == "move":
            for c in range(3):
                turb.pos[c * turb.cap + op[1]] = float(f32(op[2][c]))
        sizes.append(turb.pySize())
        cursors.append(core._turbulence_state.cursor)
    s.sync()
    return turb.channels_to_numpy(), np.array(sizes, np.int64), np.array(cursors, np.int64)


def setup_loop_pkg(m, res, dt):
    """the set-up of tools/tests/test_2025_turb.py at gridSize (res, res / 2, res / 2), its three lines that need reinitMarching
    (obstacleGradient, obstacleLevelset, createMesh: results unused in the loop) left out"""
    gs = m.vec3(res, res // 2, res // 2)
    s = m.Solver(name="main", gridSize=gs)
    s.timestep = dt
    g = dict(s=s, gs=gs, velInflow=m.vec3(0.52, 0, 0), flags=s.create(m.FlagGrid), pressure=s.create(m.RealGrid), vel=s.create(m.MACGrid))
    for name in ("k", "eps", "prod", "nuT", "strain"):
        g[name] = s.create(m.RealGrid)
    noise = s.create(m.NoiseField)
    noise.timeAnim = 0
    g["turb"] = s.create(m.TurbulenceParticleSystem, noise=noise)
    g["flags"].initDomain()
    g["flags"].fillGrid()
    for i in range(4):
        for j in range(4):
            obs = s.create(m.Sphere, center=gs * m.vec3(0.2, (i + 1) / 5.0, (j + 1) / 5.0), radius=res * 0.025)
            obs.applyToGrid(grid=g["flags"], value=m.FlagObstacle)
    g["box"] = s.create(m.Box, center=gs * m.vec3(0.05, 0.43, 0.6), size=gs * m.vec3(0.02, 0.005, 0.07))
    m.KEpsilonBcs(flags=g["flags"], k=g["k"], eps=g["eps"], intensity=0.1, nu=0.1, fillArea=True)
    return g


def step_loop_pkg(m, g, timer=None):
    """one pass of the loop of test_2025_turb.py:80-105 -> (particles after deleteInObstacle, CG iterations); timer(name, fn) may
    wrap the turbulence calls"""
    L0, mult, intensity, nu, prodMult = 0.01, 0.1, 0.1, 0.1, 2.5
    s, flags, vel, k, eps, turb, velInflow = g["s"], g["flags"], g["vel"], g["k"], g["eps"], g["turb"], g["velInflow"]
    run = timer or (lambda name, fn: fn())
    run("seed", lambda: turb.seed(g["box"], 500))
    run("advectInGrid", lambda: turb.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4))
    run("synthesize", lambda: turb.synthesize(flags=flags, octaves=1, k=k, switchLength=5, L0=L0, scale=mult, inflowBias=velInflow))
    run("deleteInObstacle", lambda: turb.deleteInObstacle(flags))
    count = turb.pySize()
    run("KEpsilonBcs", lambda: m.KEpsilonBcs(flags=flags, k=k, eps=eps, intensity=intensity, nu=nu, fillArea=False))
    m.advectSemiLagrange(flags=flags, vel=vel, grid=k, order=1)
    m.advectSemiLagrange(flags=flags, vel=vel, grid=eps, order=1)
    run("KEpsilonBcs", lambda: m.KEpsilonBcs(flags=flags, k=k, eps=eps, intensity=intensity, nu=nu, fillArea=False))
    run("KEpsilonComputeProduction", lambda: m.KEpsilonComputeProduction(vel=vel, k=k, eps=eps, prod=g["prod"], nuT=g["nuT"], strain=g["strain"], pscale=prodMult))
    run("KEpsilonSources", lambda: m.KEpsilonSources(k=k, eps=eps, prod=g["prod"]))
    run("KEpsilonGradientDiffusion", lambda: m.KEpsilonGradientDiffusion(k=k, eps=eps, vel=vel, nuT=g["nuT"], sigmaU=10.0))
    m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2, clampMode=1)
    m.setWallBcs(flags=flags, vel=vel)
    m.setInflowBcs(vel=vel, dir="xXyYzZ", value=velInflow)
    m.solvePressure(flags=flags, vel=vel, pressure=g["pressure"], cgMaxIterFac=0.5)
    iters = int(m.lastCgStats()["iterations"])
    m.setWallBcs(flags=flags, vel=vel)
    m.setInflowBcs(vel=vel, dir="xXyYzZ", value=velInflow)
    s.step()
    return count, iters
