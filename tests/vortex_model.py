"""numpy model of the vortex particle family (vortexpart.cpp:24-84, util/integrator.h:26-78, plugin/vortexplugins.cpp:29-37,
169-189, 298-310) and the seeded cases of tests/golden/vortex.npz.  Every fp32 operation is a numpy float32 operation (rounded once, never
fused); the fp64 `exp` of a pair is math.exp, the libm the reference was built against; powf / pow go through libm by ctypes.
tools/record_vortex.py asserts that this model reproduces the reference bit for bit before it writes the fixture."""
import ctypes
import ctypes.util
import hashlib
import math

import numpy as np

f32, f64 = np.float32, np.float64
PDELETE, NF_FIXED = 1 << 10, 1
EPS2 = f32(1e-6) * f32(1e-6)
FULL_LIMIT = 1200           # arrays of more elements are kept as the SHA-256 of their bytes under <key>#sha
MODES = (0, 1, 2)           # IntEuler, IntRK2, IntRK4
SEED = 3489572

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype, _libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
_libm.pow.restype, _libm.pow.argtypes = ctypes.c_double, [ctypes.c_double, ctypes.c_double]


def powf(a, b): return f32(_libm.powf(float(f32(a)), float(f32(b))))
def powd(a, b): return float(_libm.pow(float(a), float(b)))


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def put(out, key, a):
    a = np.ascontiguousarray(a)
    if a.size > FULL_LIMIT:
        out[key + "#sha"] = sha(a)
    else:
        out[key] = a


def same_as_fixture(G, key, a):
    """None if `a` is the fixture's array (or has its digest), else a description"""
    a = np.ascontiguousarray(a)
    if key in G.files:
        w = G[key]
        if w.shape != a.shape or w.dtype != a.dtype:
            return "%s: %s %s vs %s %s" % (key, a.shape, a.dtype, w.shape, w.dtype)
        u = "u%d" % a.dtype.itemsize
        d = a.view(u) != w.view(u)
        return "%s: %d of %d words differ, first at %s" % (key, int(d.sum()), d.size, np.argwhere(d)[0]) if d.any() else None
    if key + "#sha" in G.files:
        return None if np.array_equal(sha(a), G[key + "#sha"]) else "%s: digest differs" % key
    return "%s: not in the fixture" % key


# ---------------------------------------------------------------------------------------------------------
# normalize(), vectorbase.h:420-434
# ---------------------------------------------------------------------------------------------------------
def normalize(v, cnt=None):
    """-> (normalised copy [n][3], norm [n]) of float32 rows"""
    v = np.array(v, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        l = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        one = np.abs(l.astype(f64) - 1.) < f64(EPS2)
        scaled = ~one & (l > EPS2)
        nrm = np.sqrt(l)
        fac = (1. / nrm.astype(f64)).astype(f32)
    out = v.copy()
    out[scaled] = v[scaled] * fac[scaled, None]
    out[~one & ~scaled] = 0
    norm = np.where(one, f32(1), np.where(scaled, nrm, f32(0))).astype(f32)
    if cnt is not None:
        for k, m in (("branch_unit", one), ("branch_scaled", scaled), ("branch_zero", ~one & ~scaled)):
            cnt[k] = cnt.get(k, 0) + int(m.sum())
    return out, norm


# ---------------------------------------------------------------------------------------------------------
# VortexKernel, vortexpart.cpp:24-53
# ---------------------------------------------------------------------------------------------------------
def velocity(tpos, tzero, spos, sflag, vort, sigma, scale, cnt=None, bound=False):
    """u[nT][3] for targets tpos[nT][3] (tzero: targets whose u is 0) of sources spos[nS][3]; with bound=True also the per-component
    bound 2^-23 * (sum |t_i| + n * max |S_j|) of tests/test_gpu_vortex.py as a float64 array"""
    tpos, spos = np.asarray(tpos, f32).reshape(-1, 3), np.asarray(spos, f32).reshape(-1, 3)
    nT, nS = tpos.shape[0], spos.shape[0]
    c = cnt if cnt is not None else {}
    add = lambda k, v: c.__setitem__(k, c.get(k, 0) + int(v))
    vn, nrm = normalize(np.asarray(vort, f32).reshape(-1, 3), c)
    strength = nrm * f32(scale)
    sigma = np.asarray(sigma, f32).reshape(-1)
    sigma2 = sigma * sigma
    u = np.zeros((nT, 3), f32)
    live = ~np.asarray(tzero, bool).reshape(-1)
    add("zeroed_targets", (~live).sum())
    sumabs, maxabs, nterm = np.zeros((nT, 3)), np.zeros((nT, 3)), np.zeros(nT)
    px, py, pz = tpos[:, 0], tpos[:, 1], tpos[:, 2]
    with np.errstate(all="ignore"):
        for s in range(nS):
            if sflag[s] & PDELETE:
                add("deleted_sources", 1)
                continue
            rx, ry, rz = px - spos[s, 0], py - spos[s, 1], pz - spos[s, 2]
            rlen2 = (rx * rx + ry * ry) + rz * rz
            r2 = rlen2.astype(f64)
            cut = 6.0 * float(sigma2[s])
            keep = live & ~((r2 > cut) | (r2 < 1e-8))
            add("pairs", live.sum())
            add("at_cutoff_kept", (keep & (r2 == cut)).sum())
            add("ulp_beyond_cutoff", (live & (rlen2 == np.nextafter(f32(cut), f32(np.inf))) & (f64(f32(cut)) == cut)).sum())
            add("coincident", (live & (r2 < 1e-8)).sum())
            if sigma[s] == 0:
                add("sigma_zero", 1)
            idx = np.nonzero(keep)[0]
            if idx.size == 0:
                continue
            add("inside", idx.size)
            rx, ry, rz, rlen2, r2 = rx[idx], ry[idx], rz[idx], rlen2[idx], r2[idx]
            rlen = np.sqrt(rlen2)
            vx, vy, vz = vn[s]
            z = (rx * vx + ry * vy) + rz * vz
            ex = ((ry * vz) - (rz * vy)) / rlen
            ey = ((rz * vx) - (rx * vz)) / rlen
            ez = ((rx * vy) - (ry * vx)) / rlen
            rho2 = rlen2 - z * z
            big = rho2.astype(f64) > 1e-10
            add("rho2_small", (~big).sum())
            arg = (r2 * -0.5) / float(sigma2[s])
            ex64 = np.array([math.exp(a) for a in arg.tolist()], f64)
            amp = (strength[s] * np.sqrt(np.where(big, rho2, f32(0)))).astype(f64)
            vortex = np.where(big, (amp * ex64).astype(f32), f32(0)).astype(f32)
            if strength[s] != 0:
                add("underflow", (big & (np.abs(vortex) < np.finfo(f32).tiny)).sum())
            t = np.stack([vortex * ex, vortex * ey, vortex * ez], 1)
            u[idx] = u[idx] + t
            if bound:
                sumabs[idx] += np.abs(t.astype(f64))
                maxabs[idx] = np.maximum(maxabs[idx], np.abs(u[idx].astype(f64)))
                nterm[idx] += 1
    if bound:
        return u, 2.0 ** -23 * (sumabs + nterm[:, None] * maxabs)
    return u


# ---------------------------------------------------------------------------------------------------------
# integratePointSet, util/integrator.h:26-78
# ---------------------------------------------------------------------------------------------------------
def stage_update(step, x, u, x0, ut):
    """one stage's update as the kernel fuses it; step: 'euler', 'rk2a', 'full', 'rk4a', 'rk4b', 'rk4c', 'rk4d' -> (x, x0, ut)"""
    half, two, sixth = f32(0.5), f32(2), f32(1. / 6.)
    if step == "euler":
        return x + u, x0, ut
    if step == "rk2a":
        return x + half * u, x.copy(), ut
    if step == "full":
        return x0 + u, x0, ut
    if step == "rk4a":
        return x + half * u, x.copy(), u + u
    if step == "rk4b":
        return x0 + half * u, x0, ut + two * u
    if step == "rk4c":
        return x0 + u, x0, ut + two * u
    return x0 + sixth * (ut + u), x0, ut


STEPS = {0: ("euler",), 1: ("rk2a", "full"), 2: ("rk4a", "rk4b", "rk4c", "rk4d")}


def integrate(x, vel_of, mode):
    """vel_of(x) -> u; every stage's velocity pass reads the positions of the stage before"""
    if mode not in STEPS:
        raise RuntimeError("unknown integration type")
    x = np.array(x, f32).reshape(-1, 3)
    x0 = ut = None
    with np.errstate(all="ignore"):
        for step in STEPS[mode]:
            x, x0, ut = stage_update(step, x, vel_of(x), x0, ut)
    return x


def advect_self(P, scale, mode, cnt=None):
    zero = (P["flag"] & PDELETE) != 0
    return integrate(P["pos"], lambda x: velocity(x, zero, x, P["flag"], P["vorticity"], P["sigma"], scale, cnt), mode)


def apply_to_mesh(P, nodes, nflags, scale, mode, cnt=None):
    zero = (np.asarray(nflags) & NF_FIXED) != 0
    return integrate(nodes, lambda x: velocity(x, zero, P["pos"], P["flag"], P["vorticity"], P["sigma"], scale, cnt), mode)


# ---------------------------------------------------------------------------------------------------------
# the velocity / integration cases
# ---------------------------------------------------------------------------------------------------------
def _particles(rng, n, side=8.0, deleted=0.0):
    P = dict(pos=(rng.random((n, 3)) * side).astype(f32), vorticity=((rng.random((n, 3)) - 0.5) * 4).astype(f32),
             sigma=(0.4 + rng.random(n) * 1.0).astype(f32), flag=np.zeros(n, np.int32))
    if deleted and n:
        P["flag"][rng.random(n) < deleted] = PDELETE
    return P


# name -> (kind, targets, sources, seed, scale * dt, share of deleted particles, share of fixed nodes)
CASES = {}
for _q, _n in enumerate((0, 1, 63, 64, 65, 255, 256, 257, 600, 1000)):
    CASES["self%d" % _n] = ("self", _n, _n, 100 + _q, 0.25, 0.1 if _n in (65, 257, 1000) else 0.0, 0.0)
for _q, (_t, _s) in enumerate(((0, 257), (1, 1), (63, 255), (64, 256), (65, 257), (257, 0), (257, 600), (1000, 600), (1000, 1))):
    CASES["mesh%d_%d" % (_t, _s)] = ("mesh", _t, _s, 200 + _q, 0.5, 0.1 if _s in (257, 600) else 0.0, 0.15 if _t in (65, 1000) else 0.0)
CASES["edge"] = ("self", 0, 0, 0, 1.0, 0, 0)
CASES["underflow"] = ("self", 65, 65, 300, 1e-36, 0, 0)
# seeded cases beside the fixture's (tests/test_gpu_vortex.py): again around the workgroup (64 targets) and the tile (256 sources)
EXTRA_CASES = {"xself257": ("self", 257, 257, 901, 0.75, 0.05, 0.0), "xself513": ("self", 513, 513, 902, 0.25, 0.0, 0.0),
               "xmesh129_511": ("mesh", 129, 511, 903, 1.5, 0.05, 0.1), "xmesh1000_768": ("mesh", 1000, 768, 904, 0.5, 0.0, 0.0)}


def _edge_particles():
    """hand-placed groups, more than any cutoff apart: a pair exactly at rlen2 == 6 sigma2 (kept) and one an ulp beyond (skipped),
    two coincident particles, a vorticity parallel to r, a zero and a unit vorticity, sigma == 0, a deleted source"""
    one_up2 = np.nextafter(np.nextafter(f32(1), f32(2)), f32(2))
    rows = [
        # pos, vorticity, sigma, flag
        ((0, 0, 0), (0.5, -0.25, 2.0), 1.0, 0),           # the source of the cutoff pairs
        ((1, 1, 2), (0.1, 0.2, 0.3), 0.25, 0),            # rlen2 == 6 == 6 sigma2: kept
        ((-1, one_up2, 2), (0.3, 0.1, 0.2), 0.25, 0),     # rlen2 == nextafter(6): skipped
        ((30, 0, 0), (0, 0, 1.5), 1.0, 0),                # two coincident particles
        ((30, 0, 0), (1.5, 0, 0), 1.0, 0),
        ((30, 1, 0.5), (0.2, 0.2, 0.2), 0.5, 0),          # ... and one that sees both
        ((60, 0, 0), (0, 0, 3), 1.0, 0),                  # vorticity parallel to r
        ((60, 0, 1), (0, 0, -2), 1.0, 0),
        ((0, 30, 0), (0, 0, 0), 1.0, 0),                  # zero vorticity: normalize's third branch
        ((0.5, 30, 0.5), (0, 1, 0), 1.0, 0),              # unit vorticity: its first branch
        ((0, 60, 0), (1, 2, 3), 0.0, 0),                  # sigma == 0
        ((0.001, 60, 0), (3, 2, 1), 1.0, 0),
        ((0, 0, 30), (1, 1, 1), 1.0, PDELETE),            # a deleted particle: no source, no target
        ((0.5, 0.5, 30), (1, -1, 1), 1.0, 0),
    ]
    return dict(pos=np.array([r[0] for r in rows], f32), vorticity=np.array([r[1] for r in rows], f32),
                sigma=np.array([r[2] for r in rows], f32), flag=np.array([r[3] for r in rows], np.int32))


def case_inputs(name):
    """-> dict(kind, scale, P = the particles, nodes, nflags (mesh cases))"""
    kind, nT, nS, seed, scale, deleted, fixed = CASES[name] if name in CASES else EXTRA_CASES[name]
    rng = np.random.default_rng(seed)
    if name == "edge":
        return dict(kind=kind, scale=f32(scale), P=_edge_particles())
    P = _particles(rng, nS, deleted=deleted)
    if name == "underflow":
        P["vorticity"] = (P["vorticity"] * f32(1e-3)).astype(f32)
    I = dict(kind=kind, scale=f32(scale), P=P)
    if kind == "mesh":
        I["nodes"] = (rng.random((nT, 3)) * 8.0).astype(f32)
        I["nflags"] = np.where(rng.random(nT) < fixed, NF_FIXED | 2, rng.integers(0, 2, nT) * 2).astype(np.int32)
    return I


def case_targets(I):
    """(positions, zero mask) of the targets of a case"""
    if I["kind"] == "self":
        return I["P"]["pos"], (I["P"]["flag"] & PDELETE) != 0
    return I["nodes"], (I["nflags"] & NF_FIXED) != 0


def run_case(name, mode, cnt=None):
    """the end positions of the targets"""
    I = case_inputs(name)
    if I["kind"] == "self":
        return advect_self(I["P"], I["scale"], mode, cnt)
    return apply_to_mesh(I["P"], I["nodes"], I["nflags"], I["scale"], mode, cnt)


def case_velocity(name, cnt=None, bound=False):
    I = case_inputs(name)
    tp, tz = case_targets(I)
    P = I["P"]
    return velocity(tp, tz, P["pos"], P["flag"], P["vorticity"], P["sigma"], I["scale"], cnt, bound)


# ---------------------------------------------------------------------------------------------------------
# VPseedK41, vortexplugins.cpp:169-189
# ---------------------------------------------------------------------------------------------------------
class Stream(object):
    """RandomStream(3489572): MT19937 with init_genrand seeding, getReal() = float(randInt() * (1 / 4294967295))"""

    def __init__(self, cursor=0):
        self.bg = np.random.MT19937()
        self.bg._legacy_seeding(SEED)
        self.cursor = 0
        while self.cursor < cursor:
            self.real()

    def real(self):
        self.cursor += 1
        return f32(float(self.bg.random_raw(1)[0]) * (1.0 / 4294967295.0))


def inside(shape, x, y, z, is3d):
    """Box::isInside / Sphere::isInside, shapes.cpp: ('box', p0, p1) ignores z on a 2-D solver; ('sphere', centre, radius)"""
    x, y, z = f32(x), f32(y), f32(z)
    if shape[0] == "box":
        a, b = np.array(shape[1], f32), np.array(shape[2], f32)
        ok = x >= a[0] and y >= a[1] and x <= b[0] and y <= b[1]
        return bool(ok and (not is3d or (z >= a[2] and z <= b[2])))
    c, r = np.array(shape[1], f32), f32(shape[2])
    d = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
    return bool(f32(d) <= f32(float(r) * float(r)))


def seed_k41(P, st, dims, dt, shape, strength, sigma0, sigma1, probability, N, cnt=None):
    """appends to P = dict(pos, vorticity, sigma, flag) (lists of rows)"""
    sx, sy, sz = dims
    is3d = sz > 1
    strength, sigma0, sigma1, probability, N = (f32(v) for v in (strength, sigma0, sigma1, probability, N))
    s0, s1 = powf(sigma0, f32(-float(N) + 1.0)), powf(sigma1, f32(-float(N) + 1.0))
    thr = f32(probability * f32(dt))
    c = cnt if cnt is not None else {}
    for k in range(sz):
        for j in range(sy):
            for i in range(sx):
                if not inside(shape, i + 0.5, j + 0.5, k + 0.5, is3d):
                    continue
                c["cells"] = c.get("cells", 0) + 1
                if not st.real() < thr:
                    c["rejected"] = c.get("rejected", 0) + 1
                    continue
                p = st.real()
                sigma = f32(powd((1.0 - float(p)) * float(s0) + float(f32(p * s1)), 1. / (-float(N) + 1.0)))
                dz, dy, dx = st.real(), st.real(), st.real()         # the constructor's arguments are evaluated last to first
                oz, oy, ox = st.real(), st.real(), st.real()
                d, _ = normalize([[dx, dy, dz]])
                vort = (d[0] * strength) * powf(sigma, f32(-10. / 6. + float(N) / 2.0))
                P["pos"].append(np.array([f32(i) + ox, f32(j) + oy, f32(k) + oz], f32))
                P["vorticity"].append(vort.astype(f32))
                P["sigma"].append(sigma)
                P["flag"].append(0)
                c["seeded"] = c.get("seeded", 0) + 1


def new_system():
    return dict(pos=[], vorticity=[], sigma=[], flag=[])


def system_arrays(P):
    n = len(P["flag"])
    return dict(pos=np.array(P["pos"], f32).reshape(n, 3), vorticity=np.array(P["vorticity"], f32).reshape(n, 3),
                sigma=np.array(P["sigma"], f32).reshape(n), flag=np.array(P["flag"], np.int32).reshape(n))


CHANNELS = ("pos", "vorticity", "sigma", "flag")
BOX3 = ("box", (3.0, 2.0, 2.0), (8.0, 7.0, 6.0))
BALL3 = ("sphere", (6.0, 5.0, 4.0), 3.0)
BOX2 = ("box", (2.0, 2.0, 0.0), (9.0, 7.0, 1.0))
BALL2 = ("sphere", (6.0, 5.0, 0.5), 3.5)
# all cases run in this order in one process: the stream is a static of the reference.  name -> (dims, dt, calls); a call is
# (shape, strength, sigma0, sigma1, probability, N); 'reset' cases start a fresh stream (the recorder runs them first in a process)
SEED_ORDER = ("box3", "ball3", "above1", "zero", "twice", "box2", "ball2")
SEED_CASES = {
    "box3": ((12, 10, 8), 0.5, [(BOX3, 0.7, 0.2, 1.0, 0.6, 3.0)]),                      # probability * dt in between
    "ball3": ((12, 10, 8), 0.5, [(BALL3, 1.5, 0.3, 1.5, 1.0, 2.5)]),
    "above1": ((12, 10, 8), 2.0, [(BOX3, 0.3, 0.2, 1.0, 0.75, 3.0)]),                   # probability * dt = 1.5: every cell seeds
    "zero": ((12, 10, 8), 0.5, [(BALL3, 1.0, 0.2, 1.0, 0.0, 3.0)]),                     # nothing seeds, one draw per cell
    "twice": ((12, 10, 8), 0.25, [(BOX3, 1.0, 0.2, 1.0, 1.0, 3.0), (BALL3, 2.0, 0.25, 0.8, 2.0, 3.5)]),      # the stream continues
    "box2": ((12, 10, 1), 0.5, [(BOX2, 0.7, 0.2, 1.0, 1.2, 3.0)]),                      # 2-D: k = 0 only, z still gets a draw
    "ball2": ((12, 10, 1), 0.5, [(BALL2, 0.7, 0.2, 1.0, 2.0, 3.0)]),
}


def run_seed_cases(cnt=None):
    """every seed case in SEED_ORDER on one stream -> {name: (arrays, start cursor, end cursor)}"""
    st, res = Stream(), {}
    for name in SEED_ORDER:
        dims, dt, calls = SEED_CASES[name]
        P, start = new_system(), st.cursor
        c = {}
        for call in calls:
            seed_k41(P, st, dims, dt, call[0], *call[1:], cnt=c)
        if cnt is not None:
            cnt[name] = c
        res[name] = (system_arrays(P), start, st.cursor)
    return res


# ---------------------------------------------------------------------------------------------------------
# densityFromLevelset, vortexplugins.cpp:298-310; markAsFixed :29-37
# ---------------------------------------------------------------------------------------------------------
DENSITY_CASES = {"d3": ((7, 6, 5), 400, 0.8, 0.75), "d2": ((9, 8, 1), 401, 1.0, 0.5)}     # dims, seed, value, sigma


def density_inputs(name):
    (sx, sy, sz), seed, value, sigma = DENSITY_CASES[name]
    rng = np.random.default_rng(seed)
    phi = ((rng.random((sz, sy, sx)) - 0.5) * 4 * sigma).astype(f32)       # straddles -sigma and +sigma
    phi.reshape(-1)[::7] = f32(sigma)
    phi.reshape(-1)[3::11] = f32(-sigma)
    if sz >= 5:                             # the few cells inside the two border layers: below, on and between +-sigma, above
        inner = (sz - 4, sy - 4, sx - 4)
        vals = np.array([-2.0, -1.0, 0.3, 1.0, 1.5, -1.2, -0.9, 0.9], f32) * f32(sigma)
        phi[2:sz - 2, 2:sy - 2, 2:sx - 2] = np.resize(vals, int(np.prod(inner))).reshape(inner)
    return phi, f32(value), f32(sigma)


def density_from_levelset(phi, value, sigma, cnt=None):
    sz, sy, sx = phi.shape
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    border = (i < 2) | (j < 2) | (k < 2) | (i >= sx - 2) | (j >= sy - 2) | (k >= sz - 2)
    v = (0.5 * float(value) / float(sigma) * (1.0 - phi.astype(f64))).astype(f32)
    ramp = np.where(v < 0, f32(0), np.where(v > value, value, v)).astype(f32)
    out = np.where(border, f32(0), np.where(phi < -sigma, value, np.where(phi > sigma, f32(0), ramp))).astype(f32)
    if cnt is not None:
        cnt.update(border=int(border.sum()), below=int((~border & (phi < -sigma)).sum()), above=int((~border & (phi > sigma)).sum()),
                   ramp=int((~border & ~(phi < -sigma) & ~(phi > sigma)).sum()))
    return out


FIXED_BOX = ("box", (2.0, 2.0, 2.0), (6.0, 6.0, 6.0))


def fixed_inputs():
    rng = np.random.default_rng(500)
    return (rng.random((97, 3)) * 8).astype(f32), rng.integers(0, 16, 97).astype(np.int32)


def mark_as_fixed(pos, flags, shape, exclusive):
    ins = np.array([inside(shape, p[0], p[1], p[2], True) for p in pos], bool)
    return np.where(ins, flags | NF_FIXED, (flags & ~NF_FIXED) if exclusive else flags).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------
# the recorded loop: VPseedK41, advectSelf, advectInGrid with deletions and a compress() on 12 x 10 x 8
# ---------------------------------------------------------------------------------------------------------
LOOP = dict(dims=(12, 10, 8), dt=0.5, steps=3, shape=BALL3, strength=2.0, sigma0=0.3, sigma1=1.2, probability=0.5, N=3.0, scale=1.0)


def loop_grids():
    """flags with an obstacle block the particles drift into, and a constant-plus-noise MAC velocity [z][y][x][3]"""
    sx, sy, sz = LOOP["dims"]
    rng = np.random.default_rng(600)
    flags = np.full((sz, sy, sx), 1, np.int32)
    flags[0], flags[-1], flags[:, 0], flags[:, -1], flags[:, :, 0], flags[:, :, -1] = 2, 2, 2, 2, 2, 2
    flags[2:6, 3:8, 8:10] = 2
    vel = ((rng.random((sz, sy, sx, 3)) - 0.5) * 0.5).astype(f32)
    vel[..., 0] += f32(1.25)
    return flags, vel
