"""numpy / Python model of implicit density projection (source/plugin/implicitdensityprojection.cpp): copyFlagsToFlags,
markFluidAndBoundaryCells, mapMassToGrid (the ordered weight sum and knComputeDensity -- as the literal single-thread sweep and as
the order-free statement the HIP kernels implement), computeDeltaX and mapMACToPartPositions -- plus seeded input generators
(inputs are regenerated, never stored) and the scenes' loop written in the package's API.

Layout: scalar grids [z][y][x], MAC grids [z][y][x][3], particle positions [n][3]; everything fp32 / int32, every operation
rounded where the reference rounds.
"""
import numpy as np

from nbflip_model import _axes, interp_mac, interp_real

f32, f64 = np.float32, np.float64
PDELETE = 1 << 10
TypeFluid, TypeObstacle, TypeEmpty = 1, 2, 4


def copy_flags(source):
    """copyFlagsToFlags, :336-341"""
    return np.array(source, np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# markFluidAndBoundaryCells, :29-79
# ---------------------------------------------------------------------------------------------------------------------------------
def _cells(pos):
    return np.trunc(np.asarray(pos, f32)).astype(np.int64)      # toVec3i: truncation


def push_out(phi, pos):
    """:49-60 for the particles at pos: (dist, dir); dir is meaningful where dist <= 0"""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    is3d = phi.shape[0] > 1
    dist = interp_real(phi, pos)
    eps = f32(1.0e-3)
    e2 = f32(f32(2.0) * eps)
    g = np.zeros((len(pos), 3), f32)
    for c in range(3 if is3d else 2):
        hi, lo = pos.copy(), pos.copy()
        hi[:, c] = hi[:, c] + eps
        lo[:, c] = lo[:, c] - eps
        g[:, c] = (interp_real(phi, hi) - interp_real(phi, lo)).astype(f32) / e2
    dc = np.where(dist < f32(-1.0), f32(-1.0), dist).astype(f32)
    s = -(dc.astype(f64) + 1.0e-2)
    return dist, (s[:, None] * g.astype(f64)).astype(f32)


def mark_fluid_and_boundary(pos, pflag, flags, phiObs, ptype=None, exclude=0):
    """the literal loop: returns (flags, deltaX, info); info: boundary (particles inside obstacle cells), pushing (those with
    phiObs <= 0), proposals {(component, z, y, x): [(particle, cell, value), ...]} in particle order"""
    flags = np.array(flags, np.int32)
    sz, sy, sx = flags.shape
    is3d = sz > 1
    flags = np.where(flags & TypeFluid, (flags | TypeEmpty) & ~TypeFluid, flags).astype(np.int32)      # knClearFluidFlags
    assert not ((flags & TypeObstacle) != 0)[(flags & TypeEmpty) != 0].any(), "obstacle + empty cells are outside the model"
    deltaX = np.zeros((sz, sy, sx, 3), f32)
    pos = np.asarray(pos, f32).reshape(-1, 3)
    sel = (np.asarray(pflag) & PDELETE) == 0
    if ptype is not None:
        sel &= (np.asarray(ptype) & exclude) == 0
    c = _cells(pos)
    inb = sel & (c >= 0).all(axis=1) & (c[:, 0] < sx) & (c[:, 1] < sy) & (c[:, 2] < sz)
    idx = np.nonzero(inb)[0]
    ci = c[idx]
    f = flags[ci[:, 2], ci[:, 1], ci[:, 0]]
    em = (f & TypeEmpty) != 0
    flags[ci[em, 2], ci[em, 1], ci[em, 0]] = (f[em] | TypeFluid) & ~TypeEmpty
    bnd = idx[~em & ((f & TypeObstacle) != 0)]
    dist, dirs = push_out(phiObs, pos[bnd])
    proposals = {}
    pushing = 0
    for q, p in enumerate(bnd):
        if dist[q] > 0:
            continue
        pushing += 1
        i, j, k = (int(v) for v in c[p])
        for comp in range(3 if is3d else 2):
            v = dirs[q, comp]
            for e in (0, 1):
                cell = [i, j, k]
                cell[comp] += e
                if e and cell[comp] >= (sx, sy, sz)[comp]:
                    continue
                key = (comp, cell[2], cell[1], cell[0])
                proposals.setdefault(key, []).append((int(p), (i, j, k), v))
                if abs(v) > abs(deltaX[cell[2], cell[1], cell[0], comp]):
                    deltaX[cell[2], cell[1], cell[0], comp] = v
    return flags, deltaX, dict(boundary=len(bnd), pushing=pushing, proposals=proposals)


# ---------------------------------------------------------------------------------------------------------------------------------
# mapMassToGrid, :83-180
# ---------------------------------------------------------------------------------------------------------------------------------
def _ordered_scatter(nodes, w, n):
    """per node the fp32 sum of its contributions in the order given"""
    order = np.argsort(nodes, kind="stable")
    ns, ws = nodes[order], w[order]
    counts = np.bincount(ns, minlength=n)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    acc = np.zeros(n, f32)
    live = np.nonzero(counts > 0)[0]
    r = 0
    while len(live):
        acc[live] = acc[live] + ws[start[live] + r]
        r += 1
        live = live[counts[live] > r]
    return acc


def map_weights(dims, pos, pflag):
    """knMapLinear with the grids swapped as mapMassRealHelper passes them (:168): the sum of the trilinear weights of the active
    particles, per node in particle order, the corners of a particle in setInterpol's statement order (interpol.h:97-113)"""
    sx, sy, sz = dims
    pos = np.asarray(pos, f32).reshape(-1, 3)
    p = pos[(np.asarray(pflag) & PDELETE) == 0]
    g = np.zeros((sz, sy, sx), f32)
    (xi, s0, s1), (yi, t0, t1), (zi, f0, f1) = _axes(g, p)
    Z = sx * sy if sz > 1 else 0
    base = xi + sx * yi + Z * zi
    s0f0, s1f0, s0f1, s1f1 = s0 * f0, s1 * f0, s0 * f1, s1 * f1
    offs = [Z, 1 + Z, sx + Z, 1 + sx + Z, 0, 1, sx, 1 + sx]
    ws = [t0 * s0f1, t0 * s1f1, t1 * s0f1, t1 * s1f1, t0 * s0f0, t0 * s1f0, t1 * s0f0, t1 * s1f0]
    nodes = np.stack([base + o for o in offs], axis=1).reshape(-1)
    w = np.stack(ws, axis=1).astype(f32).reshape(-1)
    return _ordered_scatter(nodes, w, sx * sy * sz).reshape(sz, sy, sx)


_N = (f32(0.25), f32(0.75), f32(0.25))


def _term(l, m, n, mass):
    return f32(f32(f32(_N[l + 1] * _N[m + 1]) * _N[n + 1]) * f32(mass))


def _branch(l, m, k):
    """the reference's conditions, with the cell's own k where the loop variable n is meant: 4 / 2 / 1 as a double, double, float"""
    if (l == 0 and m == 0) or (l == 0 and k == 0) or (m == 0 and k == 0):
        return 4
    if (l != 0 and m != 0) or (l != 0 and k != 0) or (m != 0 and k != 0):
        return 2
    return 1


def _sub(d, w, br):
    if br == 1:
        return f32(d - w)
    return f32(f64(d) - f64(w) * float(br))


def _base(w, deltaX, mass):
    """:106-110 on the whole grid (cells whose upper neighbour is outside read 0 there)"""
    mass = f32(mass)
    up = np.zeros_like(deltaX)
    up[:, :, :-1, 0] = deltaX[:, :, 1:, 0]
    up[:, :-1, :, 1] = deltaX[:, 1:, :, 1]
    up[:-1, :, :, 2] = deltaX[1:, :, :, 2]
    d = (f32(1.0) - w * mass).astype(f32)
    d = (d - (((deltaX[..., 0] - up[..., 0]) + deltaX[..., 1]) - up[..., 1])).astype(f32)
    if w.shape[0] > 1:
        d = (d - (deltaX[..., 2] - up[..., 2])).astype(f32)
    return d


def _pad(a):
    return np.pad(a, 1, constant_values=0)


def _surface(f0):
    e = _pad((f0 & TypeEmpty) != 0)
    s = e[1:-1, 1:-1, :-2] | e[1:-1, 1:-1, 2:] | e[1:-1, :-2, 1:-1] | e[1:-1, 2:, 1:-1]
    if f0.shape[0] > 1:
        s = s | e[:-2, 1:-1, 1:-1] | e[2:, 1:-1, 1:-1]
    return s


def _finish(d, fluid, flip, dt, noClamp):
    d = np.where(flip, f32(0), d).astype(f32)
    if not noClamp:
        d = np.where(d < f32(-0.5), f32(-0.5), d)
        d = np.where(d > f32(0.5), f32(0.5), d)
        d = (d.astype(f32) / f32(dt)).astype(f32)
    return np.where(fluid, d, f32(0)).astype(f32)


def compute_density_serial(w, flags, deltaX, dt, mass, noClamp=False, prekernel_only=False):
    """knComputeDensity as one thread runs it: k outer, j, i inner, flags rewritten in place.  prekernel_only: every cell against
    the entry flags instead (what a kernel that does not see earlier flips computes).  Returns (density, flags, flipped)."""
    f0 = np.array(flags, np.int32)
    fl = f0.copy()
    sz, sy, sx = f0.shape
    is3d = sz > 1
    base = _base(np.asarray(w, f32), np.asarray(deltaX, f32), mass)
    surf = _surface(f0)
    fluid = (f0 & TypeFluid) != 0
    d = base.copy()
    flip = np.zeros_like(fluid)
    see = _pad(f0) if prekernel_only else None
    pl = _pad(fl)
    for k, j, i in zip(*np.nonzero(fluid)):
        v = base[k, j, i]
        if is3d:
            src = see if prekernel_only else pl
            for l in (-1, 0, 1):
                for m in (-1, 0, 1):
                    for n in (-1, 0, 1):
                        if src[k + n + 1, j + m + 1, i + l + 1] & (TypeObstacle | TypeEmpty):
                            v = _sub(v, _term(l, m, n, mass), _branch(l, m, k))
        if surf[k, j, i] and v > 0:
            fl[k, j, i] = TypeEmpty
            pl[k + 1, j + 1, i + 1] = TypeEmpty
            flip[k, j, i] = True
        d[k, j, i] = v
    return _finish(d, fluid, flip, dt, noClamp), fl, int(flip.sum())


def _chain(base, kk, seen, mass):
    """the l, m, n subtraction chain on arrays: seen(l, m, n) -> bool array of the cells whose neighbour at that offset counts"""
    d = base.copy()
    for l in (-1, 0, 1):
        for m in (-1, 0, 1):
            for n in (-1, 0, 1):
                act = seen(l, m, n)
                w = _term(l, m, n, mass)
                # _branch per cell: k == 0 only on the lowest plane
                for kzero in (False, True):
                    br = _branch(l, m, 0 if kzero else 1)
                    sel = act & ((kk == 0) == kzero)
                    if sel.any():
                        new = (d - w).astype(f32) if br == 1 else (d.astype(f64) - f64(w) * float(br)).astype(f32)
                        d = np.where(sel, new, d)
    return d


def _before(l, m, n):
    return n < 0 or (n == 0 and (m < 0 or (m == 0 and l < 0)))


def compute_density_rounds(w, flags, deltaX, dt, mass, noClamp=False):
    """the order-free statement: candidates (fluid surface cells that are positive against the entry flags; every fluid surface
    cell when mass < 0) are decided in rounds, each once none of the 13 cells swept before it is an undecided candidate; then
    every cell's value against the final flags before it and the entry flags at and after it.  Returns (density, flags, stats)."""
    f0 = np.array(flags, np.int32)
    sz, sy, sx = f0.shape
    is3d = sz > 1
    base = _base(np.asarray(w, f32), np.asarray(deltaX, f32), mass)
    surf = _surface(f0)
    fluid = (f0 & TypeFluid) != 0
    kk = np.broadcast_to(np.arange(sz)[:, None, None], f0.shape)
    fl = f0.copy()
    stats = dict(rounds=0, candidates=0)

    def view(a, l, m, n):
        p = _pad(a)
        return p[1 + n:1 + n + sz, 1 + m:1 + m + sy, 1 + l:1 + l + sx]

    def blocked(a):
        return (a & (TypeObstacle | TypeEmpty)) != 0

    if is3d:
        d0 = _chain(base, kk, lambda l, m, n: blocked(view(f0, l, m, n)), mass)
        cand = fluid & surf & ((d0 > 0) | (f32(mass) < 0))
        stats["candidates"] = int(cand.sum())
        undecided = cand.copy()
        while undecided.any():
            wait = np.zeros_like(undecided)
            for l in (-1, 0, 1):
                for m in (-1, 0, 1):
                    for n in (-1, 0):
                        if _before(l, m, n):
                            wait |= view(undecided, l, m, n)
            ready = undecided & ~wait
            v = _chain(base, kk, lambda l, m, n: blocked(view(fl, l, m, n)), mass)      # ready cells: before = final, after = entry
            fl = np.where(ready & (v > 0), TypeEmpty, fl).astype(np.int32)
            undecided &= ~ready
            stats["rounds"] += 1
        d = _chain(base, kk, lambda l, m, n: blocked(view(fl if _before(l, m, n) else f0, l, m, n)), mass)
    else:
        d = base
    flip = fluid & surf & (d > 0)
    if not is3d:
        fl = np.where(flip, TypeEmpty, fl).astype(np.int32)
    stats["flipped"] = int(flip.sum())
    return _finish(d, fluid, flip, dt, noClamp), fl, stats


def map_mass_to_grid(flags, pos, pflag, phiObs, dt, mass, noClamp=False, serial=False):
    """mapMassRealHelper, :156-175: returns (flags, density, deltaX, stats)"""
    sz, sy, sx = np.asarray(flags).shape
    fl, deltaX, info = mark_fluid_and_boundary(pos, pflag, flags, phiObs)
    w = map_weights((sx, sy, sz), pos, pflag)
    if serial:
        d, fl2, flipped = compute_density_serial(w, fl, deltaX, dt, mass, noClamp)
        stats = dict(flipped=flipped)
    else:
        d, fl2, stats = compute_density_rounds(w, fl, deltaX, dt, mass, noClamp)
    stats.update(boundary=info["boundary"], pushing=info["pushing"], marked=fl, weights=w)
    return fl2, d, deltaX, stats


# ---------------------------------------------------------------------------------------------------------------------------------
# computeDeltaX, :184-205 and mapMACToPartPositions, :207-245
# ---------------------------------------------------------------------------------------------------------------------------------
def compute_delta_x(deltaX, Lambda, flags):
    """returns (deltaX, Lambda); a lower neighbour outside the grid counts as an obstacle"""
    flags = np.asarray(flags, np.int32)
    sz, sy, sx = flags.shape
    is3d = sz > 1
    L = np.array(Lambda, f32)
    inner = np.zeros(flags.shape, bool)
    inner[(slice(1, -1) if is3d else slice(None)), 1:-1, 1:-1] = True
    L[inner & ((flags & TypeEmpty) != 0)] = 0
    out = np.array(deltaX, f32)
    obs = (flags & TypeObstacle) != 0
    for c, ax in ((0, 2), (1, 1), (2, 0)):
        if c == 2 and not is3d:
            continue
        lo_obs = np.ones_like(obs)
        lo_L = np.zeros_like(L)
        dst = [slice(None)] * 3
        src = [slice(None)] * 3
        dst[ax], src[ax] = slice(1, None), slice(None, -1)
        lo_obs[tuple(dst)] = obs[tuple(src)]
        lo_L[tuple(dst)] = L[tuple(src)]
        sel = ~obs & ~lo_obs
        out[..., c] = np.where(sel, (L - lo_L).astype(f32), out[..., c])
    return out, L


def map_mac_to_part_positions(dims, deltaX, pos, pflag, dt, ptype=None, exclude=0):
    sx, sy, sz = dims
    pos = np.array(pos, f32).reshape(-1, 3)
    sel = (np.asarray(pflag) & PDELETE) == 0
    if ptype is not None:
        sel &= (np.asarray(ptype) & exclude) == 0
    dx = interp_mac(np.asarray(deltaX, f32), pos)
    new = (pos + (dx * f32(dt)).astype(f32)).astype(f32)
    lo = np.array([1.001, 1.001, 1.001 if sz > 1 else -10.001], f32)
    hi = np.array([f32(sx) - f32(1.001), f32(sy) - f32(1.001), f32(sz) - f32(1.001) if sz > 1 else f32(10.001)], f32)
    new = np.where(new > hi, hi, new)
    new = np.where(new < lo, lo, new).astype(f32)
    return np.where(sel[:, None], new, pos).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def wall_phi(dims, bw=1):
    """phiWalls of initDomain(boundaryWidth = bw), grid.cpp:750-796"""
    sx, sy, sz = dims
    kk, jj, ii = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    sides = [ii - 0.5 - bw, sx - ii - 1.5 - bw, jj - 0.5 - bw, sy - jj - 1.5 - bw]
    if sz > 1:
        sides += [kk - 0.5 - bw, sz - kk - 1.5 - bw]
    return np.minimum.reduce([s.astype(f64) for s in sides]).astype(f32)


def domain_flags(dims, bw=1):
    sx, sy, sz = dims
    f = np.full((sz, sy, sx), TypeEmpty, np.int32)
    f[:, :, :bw + 1] = TypeObstacle
    f[:, :, sx - 1 - bw:] = TypeObstacle
    f[:, :bw + 1, :] = TypeObstacle
    f[:, sy - 1 - bw:, :] = TypeObstacle
    if sz > 1:
        f[:bw + 1] = TypeObstacle
        f[sz - 1 - bw:] = TypeObstacle
    return f


# block of obstacle cells x in [5, 7], with phiObs a function of x alone around it: -0.8, -0.3, -0.8 at the three cell centres, so that
# the particles at x = 6.25 and x = 6.75 (same y, z; mirror images about the centre of cell 6, one binade) get gradients of equal
# magnitude and opposite sign and the same distance: a tie on both x faces of cell 6
BLOCK_X = (5, 8)


def mark_inputs(dims, seed, n=600):
    """flags (walls of width 1, an obstacle block, some fluid to be cleared), phiObs, particles (random ones over and around the
    domain, many of them inside obstacle cells; deleted and excluded ones; the tie pairs), ptype"""
    sx, sy, sz = dims
    is3d = sz > 1
    rng = np.random.RandomState(seed)
    flags = domain_flags(dims)
    ys, zs = slice(3, sy - 3), (slice(3, sz - 3) if is3d else slice(None))
    flags[zs, ys, BLOCK_X[0]:BLOCK_X[1]] = TypeObstacle
    free = flags == TypeEmpty
    flags[free & (rng.uniform(size=flags.shape) < 0.3)] = TypeFluid
    phi = (wall_phi(dims) + rng.uniform(-0.2, 0.2, flags.shape)).astype(f32)
    for x, v in zip(range(BLOCK_X[0] - 1, BLOCK_X[1] + 1), (-0.1, -0.8, -0.3, -0.8, -0.1)):
        phi[:, 2:sy - 2, x] = v
    pos = rng.uniform([-1, -1, -1 if is3d else 0.2], [sx + 1, sy + 1, sz + 1 if is3d else 0.8], (n, 3))
    extra = rng.uniform([BLOCK_X[0], 3, 3 if is3d else 0.3], [BLOCK_X[1], sy - 3, sz - 3 if is3d else 0.7], (n // 4, 3))
    y0, z0 = 4.3125, (4.6875 if is3d else 0.5)
    ties = [[6.75, y0, z0], [6.25, y0, z0], [6.25, y0 + 2, z0], [6.75, y0 + 2, z0]]
    pos = np.concatenate([pos, extra])
    cy, cx = np.trunc(pos[:, 1]), np.trunc(pos[:, 0])
    pos = pos[~(((cy == 4) | (cy == 6)) & (cx >= BLOCK_X[0] - 1) & (cx <= BLOCK_X[1]))]       # the tie pairs have their rows to themselves
    pos = np.concatenate([pos, ties]).astype(f32)
    m = len(pos)
    pflag = np.where(rng.uniform(size=m) < 0.08, PDELETE, 0).astype(np.int32)
    ptype = np.where(rng.uniform(size=m) < 0.15, 4, rng.randint(0, 2, m) * 2).astype(np.int32)
    pflag[-4:] = 0
    ptype[-4:] = 0
    return dict(flags=flags, phiObs=phi, pos=pos, pflag=pflag, ptype=ptype, exclude=4)


def mass_inputs(dims, seed, per_axis=2, fill=0.6, thin=0.5):
    """a pool with a ragged surface under air, walls of width 1 and an obstacle block: per_axis^dim jittered particles per pool cell,
    thinned at random near the surface (so that surface cells stay positive and flip), plus strays inside the walls"""
    sx, sy, sz = dims
    is3d = sz > 1
    rng = np.random.RandomState(seed)
    flags = domain_flags(dims)
    flags[(slice(2, 5) if is3d else slice(None)), 2:4, BLOCK_X[0]:BLOCK_X[1]] = TypeObstacle
    phi = wall_phi(dims)
    kk, jj, ii = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    height = fill * sy + 1.5 * np.sin(ii * 0.9 + seed) + (1.2 * np.cos(kk * 1.1) if is3d else 0)
    pool = (flags == TypeEmpty) & (jj < height)
    cells = np.stack(np.nonzero(pool)[::-1], axis=1)          # x, y, z
    sub = np.stack(np.meshgrid(*[np.arange(per_axis)] * (3 if is3d else 2), indexing="ij"), axis=-1).reshape(-1, 3 if is3d else 2)
    if not is3d:
        sub = np.concatenate([sub, np.zeros((len(sub), 1), int)], axis=1)
    pos = (cells[:, None, :] + (sub[None] + rng.uniform(0.1, 0.9, (len(cells), len(sub), 3))) / per_axis).reshape(-1, 3)
    if not is3d:
        pos[:, 2] = 0.5
    near = pos[:, 1] > height[tuple(np.trunc(pos[:, ::-1]).astype(int).T)] - 2.0
    keep = ~near | (rng.uniform(size=len(pos)) > thin)
    pos = pos[keep]
    strays = rng.uniform([0.2, 0.2, 0.2 if is3d else 0.3], [sx - 0.2, 1.9, sz - 0.2 if is3d else 0.7], (len(pos) // 40 + 4, 3))
    pos = np.concatenate([pos, strays]).astype(f32)
    pos = pos[rng.permutation(len(pos))]
    pflag = np.where(rng.uniform(size=len(pos)) < 0.03, PDELETE, 0).astype(np.int32)
    flags[(flags == TypeEmpty) & (rng.uniform(size=flags.shape) < 0.1)] = TypeFluid        # stale fluid marks: cleared by the marking
    return dict(flags=flags, phiObs=phi, pos=pos, pflag=pflag, dt=0.8, mass=1.0 / per_axis ** (3 if is3d else 2))


def delta_inputs(dims, seed):
    sx, sy, sz = dims
    rng = np.random.RandomState(seed)
    flags = domain_flags(dims)
    flags[(slice(2, 5) if sz > 1 else slice(None)), 2:5, BLOCK_X[0]:BLOCK_X[1]] = TypeObstacle
    free = flags == TypeEmpty
    flags[free & (rng.uniform(size=flags.shape) < 0.6)] = TypeFluid
    return dict(flags=flags, Lambda=rng.uniform(-1, 1, flags.shape).astype(f32),
                deltaX=rng.uniform(-0.3, 0.3, flags.shape + (3,)).astype(f32))


def position_inputs(dims, seed, n=500):
    sx, sy, sz = dims
    rng = np.random.RandomState(seed)
    is3d = sz > 1
    pos = rng.uniform([0.5, 0.5, 0.5 if is3d else 0.2], [sx - 0.5, sy - 0.5, sz - 0.5 if is3d else 0.8], (n, 3)).astype(f32)      # 2-D: z stays inside the one plane
    pflag = np.where(rng.uniform(size=n) < 0.1, PDELETE, 0).astype(np.int32)
    ptype = (rng.randint(0, 4, n) * 2).astype(np.int32)
    return dict(deltaX=rng.uniform(-1.5, 1.5, (sz, sy, sx, 3)).astype(f32), pos=pos, pflag=pflag, ptype=ptype, exclude=2, dt=0.7)


D3, D2 = (13, 11, 9), (15, 12, 1)
# the fixture cases of tests/golden/idp.npz: name -> (plugin, dims, seed, options)
CASES = {
    "mark3d": ("mark", D3, 11, dict(ptype=True)), "mark3d_all": ("mark", D3, 12, dict(ptype=False)), "mark2d": ("mark", D2, 13, dict(ptype=True)),
    "mass3d": ("mass", D3, 21, dict(noClamp=False)), "mass3d_noclamp": ("mass", D3, 22, dict(noClamp=True)),
    "mass3d_b": ("mass", (12, 14, 10), 23, dict(noClamp=False)),
    "mass2d": ("mass", D2, 24, dict(noClamp=False)), "mass2d_noclamp": ("mass", D2, 25, dict(noClamp=True)),
    "delta3d": ("delta", D3, 31, {}), "delta2d": ("delta", D2, 32, {}),
    "pos3d": ("pos", D3, 41, dict(ptype=True)), "pos2d": ("pos", D2, 42, dict(ptype=False)),
}
INPUTS = {"mark": mark_inputs, "mass": mass_inputs, "delta": delta_inputs, "pos": position_inputs}


def case_inputs(name):
    kind, dims, seed, opt = CASES[name]
    return INPUTS[kind](dims, seed)


def model_case(name, serial=False):
    """the model's outputs of a fixture case, under the fixture's array names"""
    kind, dims, seed, opt = CASES[name]
    I = case_inputs(name)
    if kind == "mark":
        fl, dX, info = mark_fluid_and_boundary(I["pos"], I["pflag"], I["flags"], I["phiObs"], I["ptype"] if opt["ptype"] else None,
                                               I["exclude"] if opt["ptype"] else 0)
        return dict(flags=fl, deltaX=dX), info
    if kind == "mass":
        fl, d, dX, stats = map_mass_to_grid(I["flags"], I["pos"], I["pflag"], I["phiObs"], I["dt"], I["mass"], opt["noClamp"], serial=serial)
        return dict(flags=fl, density=d, deltaX=dX), stats
    if kind == "delta":
        dX, L = compute_delta_x(I["deltaX"], I["Lambda"], I["flags"])
        return dict(deltaX=dX, Lambda=L), {}
    pos = map_mac_to_part_positions(dims, I["deltaX"], I["pos"], I["pflag"], I["dt"], I["ptype"] if opt["ptype"] else None,
                                    I["exclude"] if opt["ptype"] else 0)
    return dict(pos=pos), {}


def random_density_case(rng):
    """a small random 3-D input of knComputeDensity: weights around 8 per cell, sparse push-out displacements"""
    dims = tuple(int(v) for v in rng.randint(4, 8, 3))
    sx, sy, sz = dims
    flags = domain_flags(dims, bw=0)
    inner = flags == TypeEmpty
    r = rng.uniform(size=flags.shape)
    flags[inner & (r < 0.65)] = TypeFluid
    flags[inner & (r > 0.92)] = TypeObstacle
    w = rng.uniform(2, 14, flags.shape).astype(f32)
    dX = np.where(rng.uniform(size=flags.shape + (3,)) < 0.1, rng.uniform(-0.4, 0.4, flags.shape + (3,)), 0).astype(f32)
    return flags, w, dX, float(rng.choice([0.125, 0.1, 1.0 / 27])), float(rng.uniform(0.3, 1.0)), bool(rng.randint(2))


# ---------------------------------------------------------------------------------------------------------------------------------
# the scenes' loop (scenes/idp_apic01_simple.py, idp_apic02_3d.py) in the package's API
# ---------------------------------------------------------------------------------------------------------------------------------
LOOPS = {"loop3d": dict(res=20, dim=3, steps=14, cfl=0.1), "loop2d": dict(res=40, dim=2, steps=24, cfl=0.04)}
LOOP_EVERY = 7          # every n-th particle is compared


def idp_loop(m, res, dim, steps, cfl=5.0, usePositionSolver=True, before_mass=None):
    """the main loop of the two scenes: same calls, same arguments, same order (cfl: the scenes' 5.0 never shortens a step of a
    small dam break; the recorded loops use a smaller one so that the adaptive dt varies).  Returns per-step dt / CG iterations / stats and the
    final fields and particles."""
    particleNumber = 2 if dim == 3 else 3
    gs = m.vec3(res, res, res if dim == 3 else 1)
    s = m.Solver(name="main", gridSize=gs, dim=dim)
    flags, vel, pressure, tmpVec3 = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.RealGrid), s.create(m.VecGrid)
    pp = s.create(m.BasicParticleSystem)
    pVel = pp.create(m.PdataVec3)
    phiObs = s.create(m.LevelsetGrid)
    apic_mass = s.create(m.MACGrid)
    cpx, cpy, cpz = pp.create(m.PdataVec3), pp.create(m.PdataVec3), pp.create(m.PdataVec3)
    density, Lambda, deltaX, flagsPos = s.create(m.RealGrid), s.create(m.RealGrid), s.create(m.MACGrid), s.create(m.FlagGrid)
    pMass = pp.create(m.PdataReal)
    mass = 1.0 / particleNumber ** dim
    s.timestep = 1
    s.frameLength = 10000000.0
    s.timestepMin = 0.01
    s.timestepMax = 1.0
    s.cfl = cfl
    flags.initDomain(boundaryWidth=1)
    if dim == 3:
        box = m.Box(parent=s, p0=gs * m.vec3(0, 0, 0.25), p1=gs * m.vec3(0.5, 0.35, 0.75))
    else:
        box = m.Box(parent=s, p0=gs * m.vec3(0, 0, 0), p1=gs * m.vec3(0.4, 0.6, 1))
    phiInit = box.computeLevelset()
    flags.updateFromLevelset(phiInit)
    m.sampleFlagsWithParticles(flags=flags, parts=pp, discretization=particleNumber, randomness=0.5)
    m.copyFlagsToFlags(flags, flagsPos)
    flags.initDomain(boundaryWidth=1, phiWalls=phiObs)
    from mantaflow_amd import plugins
    dts, it_pos, it_vel, stats = [], [], [], []
    for t in range(steps):
        s.adaptTimestep(vel.getMax())
        dts.append(s.timestep)
        pp.advectInGrid(flags=flags, vel=vel, integrationMode=2, deleteInObstacle=False, stopInObstacle=False)
        if usePositionSolver:
            m.copyFlagsToFlags(flags, flagsPos)
            if before_mass:
                before_mass(t, flagsPos, pp, phiObs, s.timestep, mass)
            m.mapMassToGrid(flags=flagsPos, density=density, parts=pp, source=pMass, deltaX=deltaX, phiObs=phiObs, dt=s.timestep,
                            particleMass=mass, noDensityClamping=False)
            stats.append(dict(plugins.mapMassToGridStats))
            m.solvePressureSystem(rhs=density, vel=vel, pressure=Lambda, flags=flagsPos, cgAccuracy=1e-3)
            it_pos.append(int(m.lastCgStats()["iterations"]))
            m.computeDeltaX(deltaX=deltaX, Lambda=Lambda, flags=flagsPos)
            m.mapMACToPartPositions(flags=flagsPos, deltaX=deltaX, parts=pp, dt=s.timestep)
        m.apicMapPartsToMAC(flags=flags, vel=vel, parts=pp, partVel=pVel, cpx=cpx, cpy=cpy, cpz=cpz, mass=apic_mass)
        m.extrapolateMACFromWeight(vel=vel, distance=2, weight=tmpVec3)
        m.markFluidCells(parts=pp, flags=flags)
        m.addGravityNoScale(flags=flags, vel=vel, gravity=(0, -0.01 if dim == 3 else -0.002, 0))
        m.setWallBcs(flags=flags, vel=vel)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure, cgAccuracy=1e-3)
        it_vel.append(int(m.lastCgStats()["iterations"]))
        m.setWallBcs(flags=flags, vel=vel)
        m.extrapolateMACSimple(flags=flags, vel=vel, distance=5)
        m.apicMapMACGridToParts(partVel=pVel, cpx=cpx, cpy=cpy, cpz=cpz, parts=pp, vel=vel, flags=flags)
        s.step()
    return dict(dt=np.array(dts, f32), it_pos=np.array(it_pos, np.int64), it_vel=np.array(it_vel, np.int64), stats=stats,
                density=density.to_numpy(), Lambda=Lambda.to_numpy(), deltaX=deltaX.to_numpy(), flags=flags.to_numpy(),
                flagsPos=flagsPos.to_numpy(), vel=vel.to_numpy(), pos=pp.get_positions()[::LOOP_EVERY], np=np.array([pp.pySize()], np.int64))
