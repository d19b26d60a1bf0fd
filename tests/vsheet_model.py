"""numpy statement of the vortex-sheet stages (include/open/manta_hip_vsheet.h): the per-triangle geometry of
mesh.h:207-215, VortexSheetMesh::calcVorticity / reinitTexCoords (vortexsheet.cpp), meshSmokeInflow, vorticitySource, smoothVorticity
and texcoordInflow (plugin/vortexplugins.cpp:41-166), in fp32 with the reference's promotion points, and the seeded case generators.
Inputs are regenerated, never stored; the reference's outputs are in tests/golden/vsheet.npz (tools/record_vsheet.py).

A mesh is meshops_model's dict (pos[n][3], normal, flags[n], tris[t][3], tflags); a sheet state is a dict of the five per-triangle
channels; a shape is ('box', p0, p1) or ('sphere', centre, radius)."""
import os

import numpy as np

import mesh_model as MM
import meshops_model as MO

f32, f64, i32 = np.float32, np.float64, np.int32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vsheet.npz")
EPS2 = f32(1e-6) * f32(1e-6)
DEFAULTS = {"vorticity": 0.0, "vorticitySmoothed": 0.0, "circulation": 0.0, "smokeAmount": 1.0, "smokeParticles": 0.0}
_rs = MM._rs


def golden():
    return np.load(GOLDEN)


# ---- vectorbase.h on rows of fp32 vectors -------------------------------------------------------------------------------------------
def cross(t, v):
    return np.stack([t[:, 1] * v[:, 2] - t[:, 2] * v[:, 1], t[:, 2] * v[:, 0] - t[:, 0] * v[:, 2], t[:, 0] * v[:, 1] - t[:, 1] * v[:, 0]], 1).astype(f32)


def norm_square(v):
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(f32)


norm3 = MO.norm3      # norm(), vectorbase.h:384-389


def normalized(v):
    """getNormalized, vectorbase.h:404-416: fac = (float)(1. / sqrt((double)l)); the epsilon branch gives the zero vector"""
    l = norm_square(v)
    with np.errstate(all="ignore"):
        fac = (1.0 / np.sqrt(l.astype(f64))).astype(f32)
        scaled = v * fac[:, None]
    out = np.where((l > EPS2)[:, None], scaled, f32(0))
    return np.where((np.abs(l.astype(f64) - 1.0) < f64(EPS2))[:, None], v, out).astype(f32)


# ---- mesh.h:207-215 -------------------------------------------------------------------------------------------------------------------
def tri_nodes(m):
    p, t = m["pos"], m["tris"]
    return p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]


def edges(m):
    p0, p1, p2 = tri_nodes(m)
    return p1 - p0, p2 - p1, p0 - p2


def face_area(m):
    p0, p1, p2 = tri_nodes(m)
    return (0.5 * norm3(cross(p1 - p0, p2 - p0)).astype(f64)).astype(f32)


def face_normal(m):
    p0, p1, p2 = tri_nodes(m)
    return normalized(cross(p1 - p0, p2 - p0))


def face_center(m):
    p0, p1, p2 = tri_nodes(m)
    return (((p0 + p1) + p2).astype(f64) / 3.0).astype(f32)


def tri_fixed(m):
    f, t = m["flags"], m["tris"]
    return ((f[t[:, 0]] & 1) | (f[t[:, 1]] & 1) | (f[t[:, 2]] & 1)) != 0


def inside(shape, p):
    """Box::isInside / Sphere::isInside (scale 1), shapes.cpp:151-154, 240-242, at rows of fp32 positions, 3-D"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    if shape[0] == "box":
        a, b = np.array(shape[1], f32), np.array(shape[2], f32)
        return (x >= a[0]) & (y >= a[1]) & (z >= a[2]) & (x <= b[0]) & (y <= b[1]) & (z <= b[2])
    c, r = np.array(shape[1], f32), f32(shape[2])
    one = f32(1)
    u, v, w = (x - c[0]) / one, (y - c[1]) / one, (z - c[2]) / one
    return (u * u + v * v + w * w).astype(f32) <= r * r


# ---- the stages -------------------------------------------------------------------------------------------------------------------------
def default_sheet(nt):
    return {k: np.full((nt, 3) if k in ("vorticity", "vorticitySmoothed", "circulation") else nt, v, f32) for k, v in DEFAULTS.items()}


def calc_vorticity(m, circulation):
    """vortexsheet.cpp:45-59 -> vorticity, smokeAmount (0 in both branches)"""
    e0, e1, e2 = edges(m)
    area = face_area(m)
    c = circulation
    with np.errstate(all="ignore"):
        v = ((c[:, 0:1] * e0 + c[:, 1:2] * e1) + c[:, 2:3] * e2) / area[:, None]
    v = np.where((area.astype(f64) < 1e-10)[:, None], f32(0), v).astype(f32)
    return v, np.zeros(len(area), f32)


def smoke_inflow(m, shape, amount, smokeAmount):
    """vortexplugins.cpp:69-75"""
    return np.where(inside(shape, face_center(m)), f32(amount), smokeAmount).astype(f32)


def acceleration(v1, v0, dt):
    """KnAcceleration with idt = (Real)(1.0 / dt); grids as [3][n] planes"""
    return ((v1 - v0) * f32(1.0 / float(f32(dt)))).astype(f32)


def vorticity_source(m, vorticity, gravity, dims, dt, vel=None, velOld=None, scale=0.1, maxAmount=0.0, mult=1.0):
    """vortexplugins.cpp:83-120 -> (vorticity, v): v is the norm after the update, before the clamp; max(v) and mean(v) are the statistics"""
    g = np.array(gravity, f32)[None]
    dt, dx = f32(dt), f32(1.0 / max(dims))
    scale, maxAmount, mult = f32(scale), f32(maxAmount), f32(mult)
    fn = face_normal(m)
    if vel is not None:
        a = MM.interpol_mac(dims, acceleration(vel, velOld, dt), np.ascontiguousarray(face_center(m).T)).T
        arg = a - g
    else:
        arg = np.repeat(-g, fn.shape[0], 0)
    source = (f32(-1.0) * cross(fn, arg)) * scale
    source = np.where(tri_fixed(m)[:, None], f32(0), source).astype(f32)
    w = vorticity * mult
    w = (w + (dt * source) / dx).astype(f32)
    v = norm3(w)
    with np.errstate(all="ignore"):
        clamp = (maxAmount > 0) & (v > maxAmount)
        w = np.where(clamp[:, None], w * (maxAmount / v)[:, None], w).astype(f32)
    return w, v


def smooth_mult(sigma):
    return f32((-0.5 / float(f32(sigma))) / float(f32(sigma)))


def smooth_args(m, opposite, sigma):
    """the fp32 arguments of the exp of vortexplugins.cpp:139 and the neighbour triangles; 0 / 0 where opposite < 0"""
    T = m["tris"].shape[0]
    c = face_center(m)
    has = opposite >= 0
    t = np.where(has, opposite // 3, 0)
    i = np.repeat(np.arange(T), 3)
    arg = (norm_square(c[t] - c[i]) * smooth_mult(sigma)).astype(f32)
    return arg, t.astype(i32), has


def smooth_weights(m, opposite, sigma):
    """the device statement: the fp64 exp of the widened argument, rounded once -> weights[3T], index[3T]"""
    arg, t, has = smooth_args(m, opposite, sigma)
    return np.where(has, np.exp(arg.astype(f64)).astype(f32), f32(0)).astype(f32), t


def smooth_iterate(weights, index, vorticity, iters, alpha):
    """vortexplugins.cpp:149-165 with the reference's indexing weights[index[idx]] -> [every iterate (before alpha)], smoothed"""
    T = vorticity.shape[0]
    v = vorticity.copy()
    idx = index.reshape(T, 3)
    its = []
    for _ in range(iters):
        s = np.ones(T, f32)
        acc = v.copy()
        for c in range(3):
            w = weights[idx[:, c]]                    # the neighbour triangle's NUMBER indexes the 3T weights
            acc = (acc + w[:, None] * v[idx[:, c]]).astype(f32)
            s = (s + w).astype(f32)
        v = (acc / s[:, None]).astype(f32)
        its.append(v.copy())
    return its, (v * f32(alpha)).astype(f32)


def smooth_iterate_by_corner(weights, index, vorticity, iters, alpha):
    """what the loop would be with weights[idx]: NOT what the reference computes (the tests show the two differ)"""
    T = vorticity.shape[0]
    v = vorticity.copy()
    idx, wt = index.reshape(T, 3), weights.reshape(T, 3)
    for _ in range(iters):
        s = np.ones(T, f32)
        acc = v.copy()
        for c in range(3):
            acc = (acc + wt[:, c:c + 1] * v[idx[:, c]]).astype(f32)
            s = (s + wt[:, c]).astype(f32)
        v = (acc / s[:, None]).astype(f32)
    return (v * f32(alpha)).astype(f32)


def get_centered(dims, vel, idx):
    sx, sy, sz = dims
    n = sx * sy * sz
    return np.array([f32(0.5) * (vel[0][idx] + vel[0][idx + 1]), f32(0.5) * (vel[1][idx] + vel[1][idx + sx]),
                     f32(0.5) * (vel[2][idx] + vel[2][idx + sx * sy])], f32) if idx + sx * sy < n else None


def inflow_cells(dims, shape):
    sx, sy, sz = dims
    k, j, i = np.meshgrid(np.arange(sz, dtype=f32), np.arange(sy, dtype=f32), np.arange(sx, dtype=f32), indexing="ij")
    p = np.stack([i.reshape(-1) + f32(0.5), j.reshape(-1) + f32(0.5), k.reshape(-1) + f32(0.5)], 1)
    return np.nonzero(inside(shape, p))[0]


def texcoord_inflow(dims, vel, shape, dt, t0, pos, tex1, tex2):
    """vortexplugins.cpp:41-66 -> t0, tex1, tex2; the serial fp32 sum in FOR_IJK order, cnt == 0 gives NaN"""
    cells = inflow_cells(dims, shape)
    assert not (cells // (dims[0] * dims[1]) == dims[2] - 1).any(), "precondition: no inside cell in the last z plane"
    mean = np.zeros(3, f32)
    for c in cells.tolist():
        mean = mean + get_centered(dims, vel, c)
    with np.errstate(all="ignore"):
        mean = mean / f32(len(cells))
    t0 = (np.array(t0, f32) - f32(dt) * mean).astype(f32)
    ins = inside(shape, pos)
    tc = (pos + t0[None]).astype(f32)
    return t0, np.where(ins[:, None], tc, tex1).astype(f32), np.where(ins[:, None], tc, tex2).astype(f32)


def reinit_tex(pos, offset):
    return (pos + np.array(offset, f32)[None]).astype(f32)


# ---- the derived bound of the one transcendental ---------------------------------------------------------------
def ulps_apart(a, b):
    """the distance of two arrays of positive finite fp32 values (or equal zeros) in units in the last place"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


WEIGHT_ULPS = 1      # float exp (< 1 ulp from exact) against fp64 exp rounded once (<= 0.5 ulp + 2^-29 ulp): neighbours at most


def weights_decided(arg):
    """the condition on a chosen input: the fp64 exp, perturbed by its last bit either way, rounds to the same fp32 value -- then the
    device's and the host's fp64 exp, both within one fp64 ulp of exact, give the same weight.  -> number of undecided weights"""
    e = np.exp(arg.astype(f64))
    lo, hi = np.nextafter(e, -np.inf), np.nextafter(e, np.inf)
    return int(((lo.astype(f32) != e.astype(f32)) | (hi.astype(f32) != e.astype(f32))).sum())


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
DIMS = (18, 17, 16)
DT = 0.5


def degenerate():
    """a bipyramid with two equatorial nodes at one position: four zero-area triangles (area < 1e-10, the normal's epsilon branch)"""
    m = MO.bipyramid(7)
    m["pos"][1] = m["pos"][0]
    return m


def open_fan():
    """a bipyramid without its lower half: the equator is a boundary (opposite < 0 on n corners)"""
    m = MO.bipyramid(9, centre=(6.0, 6.0, 6.0))
    return MO.mesh(m["pos"], m["tris"][:9])


def _at(m, centre):
    out = MO.copy_mesh(m)
    out["pos"] = (out["pos"] + (np.array(centre, f32) - out["pos"].mean(0).astype(f32))[None]).astype(f32)
    return out


MESHES = {
    "empty": lambda: MO.mesh(np.zeros((0, 3)), np.zeros((0, 3))),
    "tetra": lambda: MO.tetrahedron(centre=(5.0, 6.0, 7.0)),
    "bipyr32": lambda: MO.bipyramid(32, centre=(6.0, 6.0, 6.0)),          # 64 triangles: one wave
    "bipyr128": lambda: MO.bipyramid(128, centre=(9.0, 8.0, 7.0)),        # 256: one block
    "perm_bipyr129": lambda: MO.permuted(MO.bipyramid(129, centre=(9.0, 8.0, 7.0)), 5),      # 258: a second block, shuffled
    "sphere17": lambda: MO.sphere(17),                                    # 1064 triangles from createMesh's order
    "degenerate": degenerate,
}
OPEN_MESHES = {"strip5": lambda: _at(MO.strip(5), (6.0, 6.0, 6.0)), "open_fan": open_fan}


def with_fixed(m, name):
    """every third node fixed, at seeded places"""
    out = MO.copy_mesh(m)
    n = out["pos"].shape[0]
    out["flags"] = np.where(_rs("vs-fixed", name).uniform(size=n) < 0.3, 1 | 8, 2).astype(i32)
    return out


def sheet_state(name, nt):
    r = _rs("vs-sheet", name)
    return {"vorticity": r.uniform(-2, 2, (nt, 3)).astype(f32), "vorticitySmoothed": r.uniform(-9, 9, (nt, 3)).astype(f32),
            "circulation": r.uniform(-1, 1, (nt, 3)).astype(f32), "smokeAmount": r.uniform(0, 1, nt).astype(f32),
            "smokeParticles": r.uniform(0, 5, nt).astype(f32)}


def mac_grid(name, dims=DIMS, amp=2.0):
    """a seeded MAC grid as [3][n] planes"""
    n = dims[0] * dims[1] * dims[2]
    return _rs("vs-vel", name, dims).uniform(-amp, amp, (3, n)).astype(f32)


SMOKE_SHAPES = {"box": ("box", (0.0, 0.0, 0.0), (9.0, 8.0, 7.25)), "sphere": ("sphere", (7.0, 7.0, 7.0), 3.0), "none": ("box", (0.0, 0.0, 0.0), (0.5, 0.5, 0.5))}
# (with vel, maxAmount, mult, scale)
SOURCE_VARIANTS = {"plain": (False, 0.0, 1.0, 0.1), "vel": (True, 0.0, 1.0, 0.1), "clamped": (True, 1.5, 0.9, 0.3), "clamped_novel": (False, 0.75, 1.0, 0.2)}
GRAVITY = (0.0, -0.25, 0.03)
SMOOTH_SIGMAS = (0.2, 0.7)
SMOOTH_ITERS = (0, 1, 3)
ALPHA = 0.8
# texcoordInflow: the calls of one process, in this order (the offset is a static of the reference); the last contains no cell
INFLOW_MESH = "sphere17"
INFLOW_CALLS = (("box", (2.0, 3.0, 4.0), (9.0, 9.5, 8.0)), ("sphere", (8.5, 8.5, 5.0), 4.0), ("box", (2.0, 3.0, 4.0), (9.0, 9.5, 8.0)),
                ("box", (3.1, 3.1, 3.1), (3.4, 3.4, 3.4)))

# the recorded loop: per step meshSmokeInflow, vorticitySource(vel, velOld), smoothVorticity, VICintegration(precondition=2) into a MAC
# grid of its own, advectInGrid (RK4) with that grid, reinitTexCoords
LOOP = dict(dims=(12, 10, 8), dt=0.4, steps=3, res=9, smoke=("sphere", (4.5, 4.5, 3.0), 2.0), amount=0.6, gravity=(0.0, -0.5, 0.0), scale=0.1,
            maxAmount=0.4, mult=0.95, iters=2, sigma=0.7, alpha=0.8, vic_sigma=1.5, vic_scale=0.5, fixed=("box", (0.0, 0.0, 0.0), (12.0, 3.0, 8.0)))


def loop_inputs():
    C = LOOP
    m = MO.sphere(C["res"])
    m["flags"] = np.where(inside(C["fixed"], m["pos"]), 1, 0).astype(i32)          # markAsFixed
    n = C["dims"][0] * C["dims"][1] * C["dims"][2]
    flags = vic_flags_border(C["dims"])                                            # advectInGrid tests no flag; VICintegration does
    return m, flags


def vic_flags_border(dims):
    sx, sy, sz = dims
    f = np.full((sz, sy, sx), 1, i32)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = 2, 2, 2, 2, 2, 2
    return np.ascontiguousarray(f.reshape(-1))


def loop_velocities(step):
    """(vel, velOld) of a step: a new seeded grid every step, the previous one as velOld"""
    name = lambda q: "loop%d" % q if q >= 0 else "loop-old"
    return mac_grid(name(step), LOOP["dims"], 0.8), mac_grid(name(step - 1), LOOP["dims"], 0.8)


# ---- VICintegration, vortexplugins.cpp:192-295: the Peskin spreading --------------------------------------------------------------------
def spread(m, vorticity, flags, dims, sigma, cosine=None, want_bound=False):
    """vortexplugins.cpp:203-248 triangle by triangle in the reference's order -> vort[n][3], wnorm[T] (and, with want_bound, the derived
    per-entry bound against the reference's float cos).  `cosine` maps the fp64 argument to the fp64 cos (numpy's
    by default); the statement is this family's: the fp64 function of the widened fp32 product, rounded once to fp32.  Asserts the
    plugin's precondition: no float sum pos + i that passes the skip tests lands on the grid size."""
    cosine = cosine or np.cos
    sx, sy, sz = dims
    n = sx * sy * sz
    sigma = f32(sigma)
    sgi = int(np.ceil(sigma))
    pkfac = f32(np.pi / f64(sigma))
    T = m["tris"].shape[0]
    out, bound = np.zeros((n, 3), f32), np.zeros(n, f64)
    absacc, counts = np.zeros(n, f64), np.zeros(n, f64)
    wnorm = np.zeros(T, f32)
    if T == 0:
        return (out, wnorm, bound) if want_bound else (out, wnorm)
    pos_all, area = face_center(m), face_area(m)
    v_all = ((vorticity * area[:, None]) * f32(16.0)).astype(f32)
    off = np.arange(-sgi, sgi)
    eps = 2.0 ** -24
    for t in range(T):
        pos = pos_all[t]
        if not np.isfinite(pos).all():
            wnorm[t] = f32(np.inf)
            continue
        axes = []
        for a, size in enumerate(dims):
            fsum = (pos[a] + off.astype(f32)).astype(f32)
            ok = ~(fsum < 0) & ~((int(pos[a]) + off) >= size)
            cell = np.where(ok, fsum, 0).astype(np.int64)
            assert not (ok & (cell >= size)).any(), "precondition: a float sum pos + i rounds onto the grid size"
            centre = (off.astype(f64) + 0.5 + f64(np.floor(pos[a]))).astype(f32)
            axes.append((ok, cell, (pos[a] - centre).astype(f32)))
        (okx, cx, dx), (oky, cy, dy), (okz, cz, dz) = axes
        ok = okx[:, None, None] & oky[None, :, None] & okz[None, None, :]
        cell = (cz[None, None, :] * sy + cy[None, :, None]) * sx + cx[:, None, None]
        d = np.stack(np.broadcast_arrays(dx[:, None, None], dy[None, :, None], dz[None, None, :]), -1).reshape(-1, 3)
        ok, cell = ok.reshape(-1), cell.reshape(-1)
        ok &= (flags[np.where(ok, cell, 0)] & 1) != 0
        dl = norm3(d)
        ok &= ~(dl > sigma)
        arg = (dl * pkfac).astype(f32)
        term = 1.0 + cosine(arg.astype(f64)).astype(f32).astype(f64)
        s = f32(0)
        for q in np.nonzero(ok)[0]:                    # the i, j, k order
            s = f32(f64(s) + term[q])
        with np.errstate(divide="ignore"):
            wnorm[t] = f32(1.0 / f64(s))
        if not ok.any():
            continue
        sel = np.nonzero(ok)[0]
        w = (term[sel] * f64(wnorm[t])).astype(f32)
        add = (v_all[t][None, :] * w[:, None]).astype(f32)
        np.add.at(out, cell[sel], add)                 # in order, fp32
        if want_bound:
            N = len(sel)
            va = float(np.abs(v_all[t]).max())
            # one cos rounding per term (eps), N roundings of the sum that may each fall the other way (2 eps relative), in the numerator
            # and in the normaliser; the two final roundings of w and v * w; see DESIGN.md section 28
            rel_sum = N * eps / float(s) + 2 * N * eps
            np.add.at(bound, cell[sel], va * (float(wnorm[t]) * eps + w.astype(f64) * (rel_sum + 4 * eps)))
            np.add.at(absacc, cell[sel], va * w.astype(f64))
            np.add.at(counts, cell[sel], 1.0)
    if want_bound:                                     # and the roundings of the cell's own running sum, which may each fall the other way
        return out, wnorm, bound + 2 * eps * counts * absacc
    return out, wnorm


def spread_undecided(m, flags, dims, sigma):
    """the condition on a chosen input: with the fp64 cos moved by its last bit either way the spreading is the same bits -- then the
    device's and the host's fp64 cos, both within one fp64 ulp of exact, agree.  -> True if the input is undecided"""
    T = m["tris"].shape[0]
    vort = np.ones((T, 3), f32)
    base = spread(m, vort, flags, dims, sigma)
    for nudge in (-np.inf, np.inf):
        other = spread(m, vort, flags, dims, sigma, cosine=lambda a: np.nextafter(np.cos(a), nudge))
        if other[0].tobytes() != base[0].tobytes() or other[1].tobytes() != base[1].tobytes():
            return True
    return False


VIC_GRIDS = ((7, 6, 5), (33, 31, 29))
VIC_SIGMAS = (1.0, 1.5, 2.0, 2.5)
VIC_COUNTS = (0, 1, 63, 64, 65, 257)


def vic_flags(dims):
    """fluid inside a one-cell obstacle border, an obstacle block in the middle (on the large grid wide enough to hold a whole stencil)"""
    sx, sy, sz = dims
    f = np.full((sz, sy, sx), 1, i32)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = 2, 2, 2, 2, 2, 2
    if sx > 20:
        f[8:20, 8:20, 8:20] = 2
    else:
        f[2, 3, 3] = 2
    return np.ascontiguousarray(f.reshape(-1))


def vic_soup(dims, T, seed, reverse=False):
    """T small triangles with seeded centres: 90 of them in one cell (where T allows), some within the stencil's reach of each of the
    six walls, some in obstacle cells -- on the large grid one in the middle of the obstacle block, where no stencil cell is fluid --
    and zero-area ones; `reverse` numbers them the other way round"""
    r = _rs("vic-soup", dims, T, seed)
    sx, sy, sz = dims
    centres = r.uniform(0.6, 1.0, (T, 3)) * 0 + np.stack([r.uniform(0.3, sx - 0.3, T), r.uniform(0.3, sy - 0.3, T), r.uniform(0.3, sz - 0.3, T)], 1)
    if T >= 200:
        centres[:90] = np.array([3.0, 3.0, 2.0]) + r.uniform(0.05, 0.95, (90, 3))
        walls = [(0, 0.4), (0, sx - 0.4), (1, 0.4), (1, sy - 0.4), (2, 0.4), (2, sz - 0.4)]
        for q, (axis, at) in enumerate(walls):
            centres[100 + q, axis] = at
        centres[110] = (3.5, 3.5, 2.5) if sx <= 20 else (14.0, 14.0, 14.0)
    ext = r.uniform(0.1, 0.6, (T, 3, 3)) - 0.35
    if T >= 64:
        ext[5] = 0                                   # a zero-area triangle
        ext[40, 1] = ext[40, 0]
    pos = (centres[:, None, :] + ext).reshape(-1, 3)
    tris = np.arange(3 * T).reshape(T, 3)
    vort = r.uniform(-2, 2, (T, 3)).astype(f32)
    if reverse:
        tris, vort = tris[::-1].copy(), vort[::-1].copy()
    return MO.mesh(pos, tris), vort


def vic_cases():
    """name -> (dims, sigma, T, reverse): every sigma on both grids at 257 triangles, every count on the small grid, and the triangle
    numbers in descending spatial order"""
    cases = {}
    for dims in VIC_GRIDS:
        for sigma in VIC_SIGMAS:
            cases["g%d_s%g_t257" % (dims[0], sigma)] = (dims, sigma, 257, False)
        cases["g%d_s2_t257_rev" % dims[0]] = (dims, 2.0, 257, True)
    for T in VIC_COUNTS[:-1]:
        cases["g7_s1.5_t%d" % T] = (VIC_GRIDS[0], 1.5, T, False)
    return cases


VIC_SOLVES = ("g33_s1.5_t257", "g7_s2_t257")       # recorded with the solve, as MAC and as Vec3 velocity
VIC_SOLVE = dict(cgMaxIterFac=1.5, cgAccuracy=1e-3, scale=0.01)
