"""numpy model of the fire, wave-equation and uv-grid plugins (plugin/fire.cpp, plugin/waves.cpp, grid.cpp:573-627,
plugin/waveletturbulence.cpp:239-307): the executable statement of the fp32 / fp64 map of DESIGN.md section 15, and the seeded input
generators of the fixture tests/golden/fields.npz (inputs are regenerated here, never stored; tools/record_fields.py records the
reference's outputs).

Scalar grids are float32 / int32 [sz][sy][sx], vector grids float32 [sz][sy][sx][3].  Every function returns new arrays.  `cnt`,
where given, counts how many cells took each branch.

The model equals the reference bit for bit with one exception: `pow(x, 0.5f)` is glibc's powf there and the correctly rounded square
root here (and on the device), so `flame` may differ by 1 ulp and `heat`, which is computed from it, by the bound of heat_bound().
The fixture keeps the reference's arrays and, for those two, the cells in which the model differs (put_near / near_fixture).
"""
import hashlib

import numpy as np

f32, f64 = np.float32, np.float64
TypeFluid, TypeObstacle, TypeEmpty = 1, 2, 4
EPS = f32(1e-6)                                  # VECTOR_EPSILON, vectorbase.h:52


def _bump(cnt, key, mask):
    if cnt is not None:
        cnt[key] = cnt.get(key, 0) + int(np.count_nonzero(mask))


def shape_of(dims):
    return (dims[2], dims[1], dims[0])


def interior(shape):
    """the cells of KERNEL(bnd = 1) as a tuple of slices"""
    z = slice(1, shape[0] - 1) if shape[0] > 1 else slice(0, 1)
    return (z, slice(1, shape[1] - 1), slice(1, shape[2] - 1))


def _sh(I, dz, dy, dx):
    def mv(s, d):
        return slice(s.start + d, s.stop + d)
    return (mv(I[0], dz), mv(I[1], dy), mv(I[2], dx))


def interior_mask(shape):
    m = np.zeros(shape, bool)
    m[interior(shape)] = True
    return m


def ulp(x):
    """the spacing of float32 at |x|"""
    x = np.abs(np.asarray(x, f32))
    return (np.nextafter(x, f32(np.inf)) - x).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# fire.cpp
# ---------------------------------------------------------------------------------------------------------------------------------
def pow_half(x):
    """pow(x, 0.5f) up to powf's last bit: the correctly rounded square root with powf's special cases -0 -> +0, -inf -> +inf"""
    with np.errstate(all="ignore"):
        r = np.sqrt(x.astype(f32)).astype(f32)
    r = np.where(x == 0, f32(0), r)
    return np.where(x == -np.inf, f32(np.inf), r).astype(f32)


FIRE_DEFAULTS = dict(burningRate=0.75, flameSmoke=1.0, ignitionTemp=1.25, maxTemp=1.75, color=(0.7, 0.7, 0.7))


def process_burn(fuel, density, react, red, green, blue, heat, dt, burningRate=0.75, flameSmoke=1.0, ignitionTemp=1.25, maxTemp=1.75,
                 color=(0.7, 0.7, 0.7), cnt=None):
    """KnProcessBurn :22-64 on the interior; red / green / blue / heat may each be None.  -> dict of the grids given"""
    g = dict(fuel=fuel, density=density, react=react, red=red, green=green, blue=blue, heat=heat)
    out = {k: v.copy() for k, v in g.items() if v is not None}
    I = interior(fuel.shape)
    br, fs, it, mt, dt = f32(burningRate), f32(flameSmoke), f32(ignitionTemp), f32(maxTemp), f32(dt)
    with np.errstate(all="ignore"):
        of, os_, re = fuel[I], density[I], react[I]
        f = (of - br * dt).astype(f32)
        f = np.where(f < 0, f32(0), f).astype(f32)
        lit = of > EPS
        r = np.where(lit, (re * (f / of).astype(f32)).astype(f32), f32(0)).astype(f32)
        flame = np.where(lit, pow_half(r), f32(0)).astype(f32)
        # (origFuel < 1.0f) ? (1.0 - origFuel) * 0.5f : 0.0f -- a double expression rounded once
        emit = np.where(of < f32(1), ((1.0 - of.astype(f64)) * 0.5).astype(f32), f32(0)).astype(f32)
        emit = ((((emit + f32(0.5)).astype(f32) * (of - f).astype(f32)).astype(f32) * f32(0.1)).astype(f32) * fs).astype(f32)
        dens = (os_ + emit).astype(f32)              # clamp()'s result is dropped: not clamped
        out["fuel"][I], out["react"][I], out["density"][I] = f, r, dens
        hot = flame != 0                              # `if (heat && flame)`: a NaN is true
        if heat is not None:
            h = (((f32(1) - flame).astype(f32) * it).astype(f32) + (flame * mt).astype(f32)).astype(f32)
            out["heat"][I] = np.where(hot, h, heat[I])
        mix = emit > EPS
        factor = (dens / (os_ + emit).astype(f32)).astype(f32)
        for key, c in zip(("red", "green", "blue"), color):
            if g[key] is not None:
                v = ((g[key][I] + (f32(c) * emit).astype(f32)).astype(f32) * factor).astype(f32)
                out[key][I] = np.where(mix, v, g[key][I])
    _bump(cnt, "fuel_le_eps", ~lit)
    _bump(cnt, "fuel_ge_1", of >= f32(1))
    _bump(cnt, "fuel_clamped", (of - br * dt).astype(f32) < 0)
    _bump(cnt, "emit_le_eps", ~mix)
    _bump(cnt, "emit_gt_eps", mix)
    _bump(cnt, "density_above_1", dens > f32(1))
    _bump(cnt, "density_below_0", dens < f32(0))
    _bump(cnt, "react_zero_heat_kept", lit & ~hot)
    _bump(cnt, "heat_written", hot)
    for key in ("red", "green", "blue", "heat"):
        _bump(cnt, "absent_" + key, [g[key] is None])
    return out


def update_flame(react, flame):
    """KnUpdateFlame :78-85 on the interior"""
    out = flame.copy()
    I = interior(react.shape)
    out[I] = np.where(react[I] > 0, pow_half(react[I]), f32(0))
    return out


def heat_bound(flame, heat, ignitionTemp, maxTemp):
    """how far heat may lie from the reference's where flame is 1 ulp off: (ignitionTemp + maxTemp) * ulp(flame) for the two
    products, plus one rounding of the result"""
    return (f64(ignitionTemp) + f64(maxTemp)) * ulp(flame).astype(f64) + ulp(heat).astype(f64)


# ---------------------------------------------------------------------------------------------------------------------------------
# waves.cpp
# ---------------------------------------------------------------------------------------------------------------------------------
def _five_point(v):
    """-4. v + v(i-1) + v(i+1) + v(j-1) + v(j+1) on the interior, left to right in double"""
    I = interior(v.shape)
    d = lambda a: a.astype(f64)
    return (((-4.0 * d(v[I]) + d(v[_sh(I, 0, 0, -1)])) + d(v[_sh(I, 0, 0, 1)])) + d(v[_sh(I, 0, -1, 0)])) + d(v[_sh(I, 0, 1, 0)])


def sec_deriv_2d(v, ret):
    out = ret.copy()
    out[interior(v.shape)] = _five_point(v).astype(f32)
    return out


def total_sum64(h):
    """knTotalSum with one thread: the interior in k, j, i order, added one by one in double"""
    x = h[interior(h.shape)].astype(f64).ravel()
    return f64(np.cumsum(x)[-1]) if x.size else f64(0)


def total_sum(h):
    return f32(total_sum64(h))


def normalize_sum_to(h, target):
    with np.errstate(all="ignore"):
        factor = f32(f64(f32(target)) / total_sum64(h))
        return (h * factor).astype(f32)


def sum_margin(h):
    """(n - 1) 2^-53 sum|h|: how far any order of fp64 additions can move the sum"""
    x = h[interior(h.shape)].astype(f64)
    return (x.size - 1) * 2.0 ** -53 * np.abs(x).sum()


def make_laplace_matrix(flags):
    """MakeLaplaceMatrix, conjugategrad.h:154-187, without fractions, into cleared grids"""
    sh = flags.shape
    A0, Ai, Aj, Ak = (np.zeros(sh, f32) for _ in range(4))
    I = interior(sh)
    fl = (flags[I] & TypeFluid) != 0
    nb = [(0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0)] + ([(-1, 0, 0), (1, 0, 0)] if sh[0] > 1 else [])
    a0 = np.zeros(fl.shape, f32)
    for o in nb:
        a0 += np.where((flags[_sh(I, *o)] & TypeObstacle) == 0, f32(1), f32(0))
    A0[I] = np.where(fl, a0, f32(0))
    Ai[I] = np.where(fl & ((flags[_sh(I, 0, 0, 1)] & TypeFluid) != 0), f32(-1), f32(0))
    Aj[I] = np.where(fl & ((flags[_sh(I, 0, 1, 0)] & TypeFluid) != 0), f32(-1), f32(0))
    if sh[0] > 1:
        Ak[I] = np.where(fl & ((flags[_sh(I, 1, 0, 0)] & TypeFluid) != 0), f32(-1), f32(0))
    return A0, Ai, Aj, Ak


def wave_s(dt, cSqr):
    """Real s = dt*dt*cSqr * 0.5"""
    dt, cSqr = f32(dt), f32(cSqr)
    return f32(f64(f32(f32(dt * dt) * cSqr)) * 0.5)


def wave_system(flags, ut, utm1, s, crankNic):
    """waves.cpp:107-126: the scaled matrix and the right-hand side"""
    s = f32(s)
    A0, Ai, Aj, Ak = make_laplace_matrix(flags)
    Ai, Aj, Ak = (Ai * s).astype(f32), (Aj * s).astype(f32), (Ak * s).astype(f32)
    A0 = ((A0 * s).astype(f32).astype(f64) + 1.0).astype(f32)
    rhs = np.zeros(ut.shape, f32)
    I = interior(ut.shape)
    r = (2.0 * ut[I].astype(f64) - utm1[I].astype(f64)).astype(f32)
    if crankNic:
        r = (r.astype(f64) + f64(s) * _five_point(ut)).astype(f32)
    rhs[I] = r
    return dict(A0=A0, Ai=Ai, Aj=Aj, Ak=Ak, rhs=rhs)


# ---------------------------------------------------------------------------------------------------------------------------------
# uv grids, grid.cpp:573-627
# ---------------------------------------------------------------------------------------------------------------------------------
def reset_uv(shape, offset=None):
    k, j, i = np.meshgrid(*[np.arange(n, dtype=f32) for n in shape], indexing="ij")
    uv = np.stack([i, j, k], axis=-1).astype(f32)
    if offset is not None:
        uv = (uv + np.asarray(offset, f32)).astype(f32)
    return uv


def uv_grid_time(t, resetTime):
    with np.errstate(all="ignore"):
        return f32(np.fmod(f32(f32(t) / f32(resetTime)), f32(1)))      # fmodf is exact


def uv_ramp(t):
    w = f32(2.0 * f64(t))
    if f64(w) > 1.0:
        w = f32(2.0 - f64(w))
    return w


def uv_weight(t, dt, resetTime, index, numUvs, cnt=None):
    """the scalar part of updateUvWeight :603-619 in fp32 as written -> (weight, reset?)"""
    t, dt, resetTime = f32(t), f32(dt), f32(resetTime)
    with np.errstate(all="ignore"):
        timeOff = f32(resetTime / f32(numUvs))
        at = f32(t + f32(f32(index) * timeOff))
        lastt = uv_grid_time(f32(at - dt), resetTime)
        currt = uv_grid_time(at, resetTime)
        w = uv_ramp(currt)
        total = f32(0)
        for i in range(numUvs):
            total = f32(total + uv_ramp(uv_grid_time(f32(t + f32(f32(i) * timeOff)), resetTime)))
        if total <= EPS:
            w = f32(1)
            _bump(cnt, "total_le_eps", [True])
        else:
            w = f32(w / total)
    reset = bool(currt < lastt)
    _bump(cnt, "reset", [reset])
    _bump(cnt, "ramp_down", [f64(f32(2.0 * f64(currt))) > 1.0])
    return w, reset


def update_uv_weight(uv, t, dt, resetTime, index, numUvs, offset=None, cnt=None):
    w, reset = uv_weight(t, dt, resetTime, index, numUvs, cnt)
    out = reset_uv(uv.shape[:3], offset) if reset else uv.copy()
    out[0, 0, 0] = (w, 0, 0)
    return out


def get_uv_weight(uv):
    return f32(uv[0, 0, 0, 0])


# ---------------------------------------------------------------------------------------------------------------------------------
# extrapolateSimpleFlags, waveletturbulence.cpp:239-307
# ---------------------------------------------------------------------------------------------------------------------------------
def _neighbours(shape):
    return [(0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0)] + ([(1, 0, 0), (-1, 0, 0)] if shape[0] > 1 else [])   # (dz, dy, dx): +x -x +y -y +z -z


def extrapolate_serial(flags, val, distance=4, flagFrom=TypeFluid, flagTo=TypeObstacle):
    """the reference's loop, literally: one cell after the other in k, j, i order, in place, early exit included"""
    sh = flags.shape
    val = val.copy()
    tmp = np.zeros(sh, np.int32)
    tmp[(flags & flagFrom) != 0] = 1
    if not ((flags & flagTo) != 0).any():
        return val
    is_int = val.dtype == np.int32
    nb = _neighbours(sh)
    kr = range(1, sh[0] - 1) if sh[0] > 1 else range(1)
    for d in range(1, 1 + distance):
        for k in kr:
            for j in range(1, sh[1] - 1):
                for i in range(1, sh[2] - 1):
                    if tmp[k, j, i] != 0 or not (flags[k, j, i] & flagTo):
                        continue
                    nbs, avg = 0, (np.int32(0) if is_int else np.zeros(val.shape[3:], f32))
                    for dz, dy, dx in nb:
                        p = (k + dz, j + dy, i + dx)
                        if tmp[p] == d:
                            avg = (avg + val[p]) if is_int else (avg + val[p]).astype(f32)
                            nbs += 1
                    if nbs > 0:
                        tmp[k, j, i] = d + 1
                        val[k, j, i] = int(int(avg) / nbs) if is_int else (avg / f32(nbs)).astype(f32)   # int(): truncation toward zero
    return val


def extrapolate(flags, val, distance=4, flagFrom=TypeFluid, flagTo=TypeObstacle, cnt=None):
    """the per-pass statement: pass d reads only cells with tmp == d and writes only cells that become d + 1, so every cell of a pass
    can be computed from the state before the pass.  No early exit: without target cells no pass writes."""
    sh = flags.shape
    val = val.copy()
    tmp = np.where((flags & flagFrom) != 0, 1, 0).astype(np.int32)
    is_int = val.dtype == np.int32
    I = interior(sh)
    to = (flags[I] & flagTo) != 0
    _bump(cnt, "both_flags", ((flags[I] & flagTo) != 0) & ((flags[I] & flagFrom) != 0))
    for d in range(1, 1 + distance):
        nbs = np.zeros(to.shape, np.int32)
        acc = np.zeros(val[I].shape, val.dtype)
        for o in _neighbours(sh):
            m = tmp[_sh(I, *o)] == d
            mm = m if acc.ndim == 3 else m[..., None]
            with np.errstate(all="ignore"):
                acc = np.where(mm, (acc + val[_sh(I, *o)]).astype(val.dtype), acc)
            nbs += m
        hit = (tmp[I] == 0) & to & (nbs > 0)
        safe = np.maximum(nbs, 1)
        with np.errstate(all="ignore"):
            if is_int:
                q = (np.sign(acc) * (np.abs(acc) // safe)).astype(np.int32)         # C's truncating division
            else:
                q = (acc / (safe.astype(f32) if acc.ndim == 3 else safe.astype(f32)[..., None])).astype(f32)
        hh = hit if acc.ndim == 3 else hit[..., None]
        val[I] = np.where(hh, q, val[I])
        tmp[I] = np.where(hit, d + 1, tmp[I])
        _bump(cnt, "written_pass_%d" % d, hit)
    return val


# ---------------------------------------------------------------------------------------------------------------------------------
# the fixture: how arrays are kept, cases, seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------------
FULL_LIMIT = 4096      # arrays with more elements are kept in the fixture as the SHA-256 of their bytes


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


def put_near(out, key, ref, model):
    """recorder side, for flame / heat: the reference's array (or its digest) and the cells in which the model differs from it"""
    put(out, key, ref)
    idx = np.flatnonzero(np.ascontiguousarray(ref).view(np.uint32).ravel() != np.ascontiguousarray(model).view(np.uint32).ravel())
    out[key + "#diffidx"] = idx.astype(np.int64)
    out[key + "#diffref"] = np.ascontiguousarray(ref).ravel()[idx]
    return idx.size


def near_fixture(golden, key, a):
    """-> (message or None, flat indices, reference values there): `a` with the recorded differing cells put in must be, bit for bit,
    the reference's array"""
    idx, ref = golden[key + "#diffidx"], golden[key + "#diffref"]
    b = np.ascontiguousarray(a).copy()
    b.reshape(-1)[idx] = ref
    return same_as_fixture(golden, key, b), idx, ref


DIMS = {"g7": (7, 5, 4), "g6": (6, 6, 6), "g33": (33, 31, 29), "g2d": (12, 9, 1), "g3": (3, 3, 1)}
ALL = ("g7", "g6", "g33", "g2d", "g3")


def _seed(name, what):
    return int.from_bytes(hashlib.sha256(("fields/%s/%s" % (name, what)).encode()).digest()[:4], "little")


def _rs(name, what):
    return np.random.RandomState(_seed(name, what))


def prefill(name, what):
    """what the caller's output grids hold before a call (border cells must keep it); finite, so that it can be hashed"""
    return _rs(name, "prefill/" + what).uniform(-9, 9, shape_of(DIMS[name])).astype(f32)


# ---- fire
FIRE_DT = 0.4
FIRE_ALT = dict(burningRate=0.31, flameSmoke=2.5, ignitionTemp=0.9, maxTemp=2.3, color=(0.3, 0.6, 0.9))
OPTIONAL = ("red", "green", "blue", "heat")
# case -> (grid, the optional grids left out, parameters)
FIRE_CASES = {n + "/all": (n, (), FIRE_DEFAULTS) for n in ALL}
FIRE_CASES.update({"g7/none": ("g7", OPTIONAL, FIRE_DEFAULTS), "g6/alt": ("g6", (), FIRE_ALT), "g2d/alt": ("g2d", ("green",), FIRE_ALT)})
FIRE_CASES.update({"g7/no_" + k: ("g7", (k,), FIRE_DEFAULTS) for k in OPTIONAL})


def fire_inputs(name):
    """fuel across <= 1e-6 (zero, tiny, negative), (0, 1), >= 1; density up to 1.1 so that some cells end above 1 (the reference does
    not clamp) and slightly negative; react in [0, 1] with zeros and one -0 (pow gives +0: heat untouched); colours and heat random"""
    sh = shape_of(DIMS[name])
    r = _rs(name, "fire")
    fuel = r.uniform(0, 1.3, sh).astype(f32)
    u = r.uniform(size=sh)
    fuel[u < 0.08] = 0
    fuel[(u >= 0.08) & (u < 0.12)] = f32(5e-7)
    fuel[(u >= 0.12) & (u < 0.16)] *= f32(-0.3)
    fuel[(u >= 0.16) & (u < 0.19)] = 1
    density = r.uniform(-0.02, 1.1, sh).astype(f32)
    react = r.uniform(0, 1, sh).astype(f32)
    u = r.uniform(size=sh)
    react[u < 0.07] = 0
    react[(u >= 0.07) & (u < 0.09)] = f32(-0.0)
    g = dict(fuel=fuel, density=density, react=react)
    for k in OPTIONAL:
        g[k] = r.uniform(0, 2, sh).astype(f32)
    if name == "g3":      # the one interior cell burns, emits and ends above 1
        g["fuel"][0, 1, 1], g["density"][0, 1, 1], g["react"][0, 1, 1] = f32(0.8), f32(0.99), f32(0.6)
    return g


def run_fire(case, cnt=None):
    """-> (outputs of processBurn, flame of updateFlame on the new react over prefill)"""
    name, absent, par = FIRE_CASES[case]
    g = fire_inputs(name)
    for k in absent:
        g[k] = None
    out = process_burn(g["fuel"], g["density"], g["react"], g["red"], g["green"], g["blue"], g["heat"], FIRE_DT, cnt=cnt, **par)
    return out, update_flame(out["react"], prefill(name, "flame"))


def fire_flame(case):
    """the flame of processBurn's interior (not an output of the plugin): what heat_bound() needs"""
    out, _ = run_fire(case)
    return update_flame(out["react"], np.zeros_like(out["react"]))


# ---- waves
WAVE_DT, WAVE_CSQR = 0.9, 0.12
SUM_KINDS = ("exact", "random")
SUM_TARGET = 3.5


def secderiv_input(name):
    return _rs(name, "secderiv").uniform(-2, 2, shape_of(DIMS[name])).astype(f32)


def sum_input(name, kind):
    """exact: multiples of 2^-6 in [-1, 4] -- every fp64 partial sum is exact, so any order gives the same sum; random: uniform"""
    sh = shape_of(DIMS[name])
    r = _rs(name, "sum/" + kind)
    if kind == "exact":
        return (r.randint(-64, 257, sh) / 64.0).astype(f32)
    return r.uniform(-1, 3, sh).astype(f32)


def wave_flags(name, obstacles=True):
    """initDomain + fillGrid, plus (obstacles) 15 % obstacle and 10 % empty cells inside"""
    sh = shape_of(DIMS[name]) if isinstance(name, str) else shape_of(name)
    flags = np.full(sh, TypeObstacle, np.int32)
    I = interior(sh)
    inner = np.full(flags[I].shape, TypeFluid, np.int32)
    if obstacles:
        r = _rs(str(name), "waveflags")
        u = r.uniform(size=inner.shape)
        inner[u < 0.15] = TypeObstacle
        inner[(u >= 0.15) & (u < 0.25)] = TypeEmpty
    flags[I] = inner
    return flags


def wave_inputs(name):
    sh = shape_of(DIMS[name])
    r = _rs(name, "wave")
    return dict(flags=wave_flags(name), ut=r.uniform(-1, 1, sh).astype(f32), utm1=r.uniform(-1, 1, sh).astype(f32))


def run_wave_system(name, crankNic):
    I = wave_inputs(name)
    return wave_system(I["flags"], I["ut"], I["utm1"], wave_s(WAVE_DT, WAVE_CSQR), crankNic)


CG_DIMS = {"cg2d": (20, 16, 1), "cg3d": (12, 10, 8)}
CG_DT, CG_CSQR = 3.0, 0.9         # s = 4.05: a system far enough from the identity for CG to take a dozen iterations


def cg_inputs(name):
    """a bump with noise, and a slightly different previous state"""
    dims = CG_DIMS[name]
    sh = shape_of(dims)
    r = _rs(name, "cg")
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, n) if n > 1 else np.zeros(1) for n in sh], indexing="ij")
    bump = np.exp(-4 * (x * x + y * y + z * z))
    ut = (bump + 0.05 * r.uniform(-1, 1, sh)).astype(f32)
    utm1 = (0.9 * bump + 0.05 * r.uniform(-1, 1, sh)).astype(f32)
    return dict(dims=dims, flags=wave_flags(dims, obstacles=False), ut=ut, utm1=utm1)


# ---- uv
UV_OFFSETS = {"none": None, "off": (0.5, -1.25, 2.0)}
UV_DT, UV_RESET = 0.5, 11.0
# every (numUvs, step, index) of 25 steps of dt 0.5 with resetTime 11: resets, both halves of the ramp, and (numUvs = 1, t = 0) the
# uvWTotal <= 1e-6 branch
UVW_SCALARS = [(n, step, i) for n in (1, 2, 3) for step in range(25) for i in range(n)]
# the grid-level cases: (grid, offset, numUvs, step, index)
UVW_GRID_CASES = {"eps_branch": ("g7", "none", 1, 0, 0), "plain": ("g7", "off", 3, 5, 1), "reset": ("g7", "off", 1, 22, 0),
                  "reset2d": ("g2d", "none", 2, 11, 1), "reset_g33": ("g33", "off", 3, 22, 0)}


def uv_time(step):
    """the solver's timeTotal after `step` steps of UV_DT (frameLength 1: every second step snaps to the frame number)"""
    return f32(step * UV_DT)


def uv_prefill(name):
    return _rs(name, "uv").uniform(-5, 40, shape_of(DIMS[name]) + (3,)).astype(f32)


def run_uvw_grid(case, cnt=None):
    name, off, n, step, i = UVW_GRID_CASES[case]
    return update_uv_weight(uv_prefill(name), uv_time(step), UV_DT, UV_RESET, i, n, UV_OFFSETS[off], cnt)


# ---- extrapolateSimpleFlags
def extrap_flags(name, kind):
    """random: fluid with 15 % obstacles inside an obstacle border; blob: an obstacle block deeper than any distance used, in fluid;
    notarget: fluid and empty only; both: as random, with some cells carrying both flags"""
    sh = shape_of(DIMS[name])
    r = _rs(name, "extrapflags/" + kind)
    flags = np.full(sh, TypeObstacle, np.int32)
    I = interior(sh)
    inner = np.full(flags[I].shape, TypeFluid, np.int32)
    u = r.uniform(size=inner.shape)
    if kind in ("random", "both"):
        inner[u < 0.15] = TypeObstacle
        if kind == "both":
            inner[(u >= 0.15) & (u < 0.22)] = TypeFluid | TypeObstacle
    elif kind == "blob":
        c = [n // 2 for n in inner.shape]
        inner[max(c[0] - 7, 0):c[0] + 8, max(c[1] - 7, 0):c[1] + 8, max(c[2] - 7, 0):c[2] + 8] = TypeObstacle
    flags[I] = inner
    if kind == "notarget":
        flags[:] = np.where(r.uniform(size=sh) < 0.3, TypeEmpty, TypeFluid)
    return flags


def extrap_val(name, vtype):
    sh = shape_of(DIMS[name])
    r = _rs(name, "extrapval/" + vtype)
    if vtype == "int":
        return r.randint(-50, 51, sh).astype(np.int32)
    if vtype == "flag":
        return extrap_flags(name, "random").copy()
    return r.uniform(-3, 3, sh + ((3,) if vtype == "vec" else ())).astype(f32)


# case -> (grid, flags kind, value type, distance, flagFrom, flagTo)
EXTRAP_CASES = {}
for _n in ALL:
    for _t in ("real", "int", "vec"):
        EXTRAP_CASES["%s/random/%s/4" % (_n, _t)] = (_n, "random", _t, 4, TypeFluid, TypeObstacle)
for _d in (0, 1, 6):
    EXTRAP_CASES["g33/blob/real/%d" % _d] = ("g33", "blob", "real", _d, TypeFluid, TypeObstacle)
    EXTRAP_CASES["g7/random/vec/%d" % _d] = ("g7", "random", "vec", _d, TypeFluid, TypeObstacle)
EXTRAP_CASES["g33/blob/vec/4"] = ("g33", "blob", "vec", 4, TypeFluid, TypeObstacle)
# the two calls of scenes/waveletTurbulenceObs.py: obstacle flags grow into the fluid, then energy from fluid into obstacles
EXTRAP_CASES["g33/scene/flag/2"] = ("g33", "random", "flag", 2, TypeObstacle, TypeFluid)
EXTRAP_CASES["g2d/scene/flag/2"] = ("g2d", "random", "flag", 2, TypeObstacle, TypeFluid)
EXTRAP_CASES["g33/scene/real/6"] = ("g33", "random", "real", 6, TypeFluid, TypeObstacle)
EXTRAP_CASES["g6/both/real/4"] = ("g6", "both", "real", 4, TypeFluid, TypeObstacle)
EXTRAP_CASES["g33/both/int/4"] = ("g33", "both", "int", 4, TypeFluid, TypeObstacle)
EXTRAP_CASES["g7/notarget/real/4"] = ("g7", "notarget", "real", 4, TypeFluid, TypeObstacle)
EXTRAP_CASES["g2d/notarget/vec/4"] = ("g2d", "notarget", "vec", 4, TypeFluid, TypeObstacle)


def extrap_inputs(case):
    name, kind, vtype, dist, ff, ft = EXTRAP_CASES[case]
    return extrap_flags(name, kind), extrap_val(name, vtype), dist, ff, ft


def run_extrap(case, cnt=None):
    flags, val, dist, ff, ft = extrap_inputs(case)
    return extrapolate(flags, val, dist, ff, ft, cnt)


def random_extrap_case(seed):
    """a small random case of the serial / per-pass equivalence test"""
    r = np.random.RandomState(seed)
    two_d = r.uniform() < 0.4
    sh = (1 if two_d else r.randint(3, 6), r.randint(3, 8), r.randint(3, 8))
    bits = np.array([TypeFluid, TypeObstacle, TypeEmpty, TypeFluid | TypeObstacle], np.int32)
    flags = bits[r.choice(4, size=sh, p=[0.45, 0.4, 0.1, 0.05])]
    vtype = ("real", "int", "vec")[seed % 3]
    if vtype == "int":
        val = r.randint(-50, 51, sh).astype(np.int32)
    else:
        val = r.uniform(-3, 3, sh + ((3,) if vtype == "vec" else ())).astype(f32)
    ff, ft = ((TypeFluid, TypeObstacle), (TypeObstacle, TypeFluid), (TypeEmpty, TypeFluid | TypeObstacle))[(seed // 3) % 3]
    return flags, val, int(r.randint(0, 6)), ff, ft


# ---- initVortexVelocity
VORTEX_CASES = {"v2d": (16, 16, 1), "v3d": (9, 7, 5)}


def vortex_inputs(name):
    """phiObs of test_1040 (minus a sphere's level set: >= -1 outside radius + 1 ... the inside of the sphere plus one cell), with
    a vel pre-filled so that untouched cells and the z component show"""
    dims = VORTEX_CASES[name]
    sh = shape_of(dims)
    center = tuple(f32(0.5 * n) for n in dims)
    radius = f32(0.4 * dims[0])
    k, j, i = np.meshgrid(*[np.arange(n, dtype=f64) + 0.5 for n in sh], indexing="ij")
    dist = np.sqrt((i - center[0]) ** 2 + (j - center[1]) ** 2 + ((k - center[2]) ** 2 if sh[0] > 1 else 0))
    phi = (-(dist - f64(radius))).astype(f32)
    vel = _rs(name, "vortexvel").uniform(-1, 1, sh + (3,)).astype(f32)
    return dict(dims=dims, phiObs=phi, vel=vel, center=center, radius=radius)


# ---------------------------------------------------------------------------------------------------------------------------------
# the four loops, through the package (`m` is the manta module); tools/record_fields.py runs the same loops against the reference's
# classes (tools/fields_record.cpp).  The reference's scripts do not travel with the tests, so the loops are stated again here.
# ---------------------------------------------------------------------------------------------------------------------------------
WAVE_LOOP = dict(dims=(23, 19, 1), steps=12, switch_at=5, dt=0.9, cSqr=0.12)       # explicit steps 0..5, implicit steps 6..11


def wave_loop_h0():
    """the script's Box(p0 = gs * 0.3, p1 = gs * 0.5) applied with value 1: the cells whose centre lies inside"""
    sx, sy, _ = WAVE_LOOP["dims"]
    j, i = np.meshgrid(np.arange(sy) + 0.5, np.arange(sx) + 0.5, indexing="ij")
    inside = (i >= f32(sx * 0.3)) & (i <= f32(sx * 0.5)) & (j >= f32(sy * 0.3)) & (j <= f32(sy * 0.5))
    return inside.astype(f32)[None]


def wave_loop_vel_factor():
    """`cSqr * s.timestep` as the reference's Python evaluates it: the timestep property reads back a Real"""
    return f32(WAVE_LOOP["cSqr"] * float(f32(WAVE_LOOP["dt"])))


def wave_loop_pkg(m):
    """tools/tests/test_1030_waveeq.py at 23 x 19, 12 steps"""
    C = WAVE_LOOP
    gs = m.vec3(*C["dims"])
    s = m.Solver(name="main", gridSize=gs, dim=2)
    implicit = False
    s.timestep = C["dt"]
    cSqr = C["cSqr"]
    h, hprev, hnew, curv, vel = (s.create(m.RealGrid) for _ in range(5))
    flags = s.create(m.FlagGrid)
    flags.initDomain()
    flags.fillGrid()
    source = s.create(m.Box, p0=gs * m.vec3(0.3, 0.3, 0.3), p1=gs * m.vec3(0.5, 0.5, 0.5))
    source.applyToGrid(grid=h, value=1)
    h0 = h.to_numpy()
    hprev.copyFrom(h)
    mass, its = [], []
    for t in range(C["steps"]):
        mass.append(m.totalSum(height=h))
        if implicit:
            m.cgSolveWE(flags=flags, ut=h, utm1=hprev, out=hnew, cSqr=cSqr, crankNic=False)
            its.append(m.lastCgStats()["iterations"])
        else:
            m.calcSecDeriv2d(h, curv)
            # the script writes cSqr * s.timestep; the reference's property reads back the Real, the package's attribute keeps the
            # Python double it was given, and the two products can differ in the last bit of the Real they become
            vel.addScaled(curv, cSqr * float(f32(s.timestep)))
            h.addScaled(vel, s.timestep)
            its.append(-1)
            if t >= C["switch_at"]:
                implicit = True
        m.normalizeSumTo(h, mass[-1])
        s.step()
    return dict(h0=h0, mass=np.array(mass, f32), iterations=np.array(its, np.int64), h=h.to_numpy(), vel=vel.to_numpy())


UV_LOOP = dict(dims=(20, 30, 1), uvs=3, steps=20, dt=0.5, resetTime=11.0)


def uv_loop_vel():
    """the script's velocity comes from a pressure solve, which is not under test: a seeded swirl of up to 2.5 cells per step, with
    the walls' normal components set by setWallBcs on both sides"""
    sx, sy, _ = UV_LOOP["dims"]
    r = _rs("uvloop", "vel")
    j, i = np.meshgrid(np.arange(sy), np.arange(sx), indexing="ij")
    v = np.zeros((1, sy, sx, 3), f32)
    v[0, ..., 0] = 2.0 * np.sin(i * 0.4) * np.cos(j * 0.3) + 0.5 * r.uniform(-1, 1, (sy, sx))
    v[0, ..., 1] = -1.5 * np.cos(i * 0.35) * np.sin(j * 0.25) + 0.5 * r.uniform(-1, 1, (sy, sx))
    return v


def uv_loop_pkg(m):
    """tools/tests/test_1020_uvs.py's main loop at 20 x 30 with 3 uv grids"""
    C = UV_LOOP
    sm = m.Solver(name="main", gridSize=m.vec3(*C["dims"]), dim=2)
    sm.timestep = C["dt"]
    flags = sm.create(m.FlagGrid)
    flags.initDomain()
    flags.fillGrid()
    uv = []
    for i in range(C["uvs"]):
        uv.append(sm.create(m.VecGrid))
        m.resetUvGrid(uv[i])
    vel = sm.create(m.MACGrid)
    vel.from_numpy(uv_loop_vel())
    weights = []
    for t in range(C["steps"]):
        for i in range(C["uvs"]):
            m.advectSemiLagrange(flags=flags, vel=vel, grid=uv[i], order=1)
            m.updateUvWeight(resetTime=C["resetTime"], index=i, numUvs=C["uvs"], uv=uv[i])
            weights.append(m.getUvWeight(uv[i]))
        sm.step()
    return dict(uv=[g.to_numpy() for g in uv], weights=np.array(weights, f32).reshape(C["steps"], C["uvs"]))


BND_LOOP = dict(res=16, steps=10)


def bnd_loop_pkg(m):
    """tools/tests/test_1040_secOrderBnd.py (new_BC) at 16 x 16"""
    res = BND_LOOP["res"]
    gs = m.vec3(res, res, 1)
    s = m.FluidSolver(name="main", gridSize=gs, dim=2)
    s.timestep = 1
    flags, vel, pressure = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.RealGrid)
    fractions, density = s.create(m.MACGrid), s.create(m.RealGrid)
    flags.initDomain()
    center = gs * m.vec3(0.5, 0.5, 0.5)
    radius = res * 0.4
    sphere = s.create(m.Sphere, center=center, radius=radius)
    phiObs = sphere.computeLevelset()
    phiObs.multConst(-1)
    m.initVortexVelocity(phiObs=phiObs, vel=vel, center=center, radius=radius)
    m.updateFractions(flags=flags, phiObs=phiObs, fractions=fractions)
    m.setObstacleFlags(flags=flags, phiObs=phiObs, fractions=fractions)
    flags.fillGrid()
    its = []
    for t in range(BND_LOOP["steps"]):
        m.advectSemiLagrange(flags=flags, vel=vel, grid=density, order=2, orderSpace=1, clampMode=1)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2, strength=1.0, clampMode=1)
        m.setWallBcs(flags=flags, vel=vel, fractions=fractions, phiObs=phiObs)
        m.extrapolateMACSimple(flags=flags, vel=vel, distance=1)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure, fractions=fractions)
        its.append(m.lastCgStats()["iterations"])
        m.setWallBcs(flags=flags, vel=vel, fractions=fractions, phiObs=phiObs)
        m.extrapolateMACSimple(flags=flags, vel=vel, distance=1)
        s.step()
    return dict(fractions=fractions.to_numpy(), vel=vel.to_numpy(), iterations=np.array(its, np.int64))


FIRE_LOOP = dict(res=16, steps=6, box=((6, 10), (1, 4), (6, 10)))       # the source box as x, y, z cell ranges
FIRE_LOOP_GRIDS = ("density", "heat", "fuel", "react", "flame", "pressure")


def fire_loop_sources():
    """the scene's four densityInflow calls (not under test) are replaced on both sides by copies of seeded random fields into the
    source box: (mask, [density, heat, fuel, react])"""
    res = FIRE_LOOP["res"]
    (x0, x1), (y0, y1), (z0, z1) = FIRE_LOOP["box"]
    mask = np.zeros((res, res, res), np.int32)
    mask[z0:z1, y0:y1, x0:x1] = 1
    r = _rs("fireloop", "sources")
    return mask, [r.uniform(0.3, 1.0, mask.shape).astype(f32) for _ in range(4)]


def fire_loop_params():
    """the scene's numbers as the reference's Python hands them to the Reals: dt0, frameLength, timestepMin, timestepMax, cfl, the y
    components of gravity * smokeDensity and gravity * smokeTempDiff, vortGlobal, vortFlames"""
    tmin, tmax = f32(0.2), f32(2.0)
    return np.array([(float(tmax) + float(tmin)) * 0.5, 1.2, tmin, tmax, 3.0, -0.0981 * -0.001, -0.0981 * 0.1, 0.1, 0.5], f32)


def fire_loop_pkg(m):
    """scenes/fire.py's loop at 16^3, 6 steps"""
    res = FIRE_LOOP["res"]
    gs = m.vec3(res, res, res)
    s = m.Solver(name="main", gridSize=gs, dim=3)
    smokeDensity, smokeTempDiff = -0.001, 0.1
    # the reference's solver attributes are Reals: what the script assigns is rounded to fp32 and read back so.  The package's are
    # plain Python attributes and adaptTimestep uses frameLength as the double it was given, so the scene's 1.2 is written here as
    # the Real it becomes in the reference (with the double, dt = (frameLength - timePerFrame) + 1e-4 lands one ulp lower)
    s.frameLength = float(f32(1.2))
    s.timestepMin = float(f32(0.2))
    s.timestepMax = 2.0
    s.cfl = 3.0
    s.timestep = (s.timestepMax + s.timestepMin) * 0.5
    flags, vel = s.create(m.FlagGrid), s.create(m.MACGrid)
    density, react, fuel, heat, flame, pressure = (s.create(m.RealGrid) for _ in range(6))
    gravity = m.vec3(0, -0.0981, 0)
    vortGlobal, vortFlames = 0.1, 0.5
    bWidth = 1
    flags.initDomain(boundaryWidth=bWidth)
    flags.fillGrid()
    m.setOpenBound(flags, bWidth, 'yY', m.FlagOutflow | m.FlagEmpty)
    mask, src = fire_loop_sources()
    dts, its = [], []
    for t in range(FIRE_LOOP["steps"]):
        maxvel = vel.getMax()
        s.adaptTimestep(maxvel)
        dts.append(s.getDt())
        for g, a in zip((density, heat, fuel, react), src):
            g.from_numpy(np.where(mask != 0, a, g.to_numpy()))
        m.processBurn(fuel=fuel, density=density, react=react, heat=heat)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=density, order=2)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=heat, order=2)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=fuel, order=2)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=react, order=2)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2)
        m.resetOutflow(flags=flags, real=density)
        flame.copyFrom(fuel)
        flame.multConst(vortFlames)
        m.vorticityConfinement(vel=vel, flags=flags, strength=vortGlobal, strengthCell=flame)
        m.addBuoyancy(flags=flags, density=density, vel=vel, gravity=(gravity * smokeDensity))
        m.addBuoyancy(flags=flags, density=heat, vel=vel, gravity=(gravity * smokeTempDiff))
        m.setWallBcs(flags=flags, vel=vel)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure)
        its.append(m.lastCgStats()["iterations"])
        m.updateFlame(react=react, flame=flame)
        s.step()
    out = dict(dts=np.array(dts, f32), iterations=np.array(its, np.int64), vel=vel.to_numpy())
    for k, g in zip(FIRE_LOOP_GRIDS, (density, heat, fuel, react, flame, pressure)):
        out[k] = g.to_numpy()
    return out
