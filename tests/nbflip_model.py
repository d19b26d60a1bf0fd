"""numpy / Python model of the narrow-band FLIP additions: adjustNumber (the literal serial loop with kill()'s mid-loop compress,
and the order-free segmented statement the HIP kernels implement), the particle system's compress, the buffered insertion,
combineGridVel, Grid::setBoundNeumann, LevelsetGrid::initFromFlags -- plus seeded input generators (inputs are regenerated,
never stored) and the narrow-band loops written in the package's API.

Layout: scalar grids [z][y][x], Vec3 / MAC grids [z][y][x][3], particle positions [n][3]; everything fp32 / int32, every
operation rounded where the reference rounds (plugin/flip.cpp:197-262, 748-776, particle.h:401-427, 614-663, particle.cpp:341-369,
grid.cpp:640-669, levelset.cpp:231-238, util/interpol.h).
"""
import numpy as np

f32 = np.float32
PNEW, PDELETE, PINVALID = 1, 1 << 10, 1 << 30
TypeFluid, TypeObstacle, TypeEmpty = 1, 2, 4
DELETE_PART = 20


# ---------------------------------------------------------------------------------------------------------------------------------
# interpolation, util/interpol.h
# ---------------------------------------------------------------------------------------------------------------------------------
def _index(p, size, upper_on_index=False, clamp_upper=True):
    """BUILD_INDEX on one axis for p = pos - 0.5 (or BUILD_INDEX_SHIFT for p = pos): cell, weight of it, weight of the next"""
    p = np.asarray(p, f32)
    with np.errstate(invalid="ignore"):
        xi = p.astype(np.int64)            # truncation
    w1 = (p - xi.astype(f32)).astype(f32)
    w0 = (1.0 - w1.astype(np.float64)).astype(f32)
    lo = p < f32(0)
    xi = np.where(lo, 0, xi); w0 = np.where(lo, f32(1), w0); w1 = np.where(lo, f32(0), w1)
    if clamp_upper:
        hi = (xi >= size - 1) if upper_on_index else (p >= f32(size - 1))
        xi = np.where(hi, size - 2, xi); w0 = np.where(hi, f32(0), w0); w1 = np.where(hi, f32(1), w1)
    return xi, w0.astype(f32), w1.astype(f32)


def _tri(g, X, Y, Z):
    """the 8-corner (4 in 2-D: both z corners are plane 0) sum in the reference's association order, interpol.h:77-80"""
    (xi, s0, s1), (yi, t0, t1), (zi, f0, f1) = X, Y, Z
    sz = g.shape[0]
    z1 = zi + 1 if sz > 1 else zi
    a = (g[zi, yi, xi] * t0 + g[zi, yi + 1, xi] * t1) * s0 + (g[zi, yi, xi + 1] * t0 + g[zi, yi + 1, xi + 1] * t1) * s1
    b = (g[z1, yi, xi] * t0 + g[z1, yi + 1, xi] * t1) * s0 + (g[z1, yi, xi + 1] * t0 + g[z1, yi + 1, xi + 1] * t1) * s1
    return (a * f0 + b * f1).astype(f32)


def _axes(g, pos, shift=(False, False, False)):
    sz, sy, sx = g.shape[:3]
    out = []
    for a, size in enumerate((sx, sy, sz)):
        p = pos[:, a].astype(f32)
        if shift[a]:
            out.append(_index(p, size, upper_on_index=True, clamp_upper=(a < 2 or sz > 1)))
        else:
            out.append(_index((p - f32(0.5)).astype(f32), size, clamp_upper=(a < 2 or sz > 1)))
    return out


def interp_real(g, pos):
    """Grid<Real>::getInterpolated"""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    return _tri(np.asarray(g, f32), *_axes(g, pos))


def interp_vec(g, pos):
    """Grid<Vec3>::getInterpolated: the scalar formula per component"""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    ax = _axes(g, pos)
    return np.stack([_tri(np.ascontiguousarray(g[..., c]), *ax) for c in range(3)], axis=1)


def interp_mac(g, pos):
    """MACGrid::getInterpolated -> interpolMAC, interpol.h:131-164: component c uses the shifted index on axis c"""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    out = []
    for c in range(3):
        ax = _axes(g, pos, shift=tuple(a == c for a in range(3)))
        out.append(_tri(np.ascontiguousarray(g[..., c]), *ax))
    return np.stack(out, axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# grid operations
# ---------------------------------------------------------------------------------------------------------------------------------
def set_bound_neumann(g, w):
    """knSetBoundaryNeumann, grid.cpp:640-669 (grids of at least 2w+3 cells per axis: every source cell is an inner cell)"""
    g = np.array(g)
    sz, sy, sx = g.shape[:3]
    is3d = sz > 1
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    si, sj, sk = i.copy(), j.copy(), k.copy()
    si[i <= w] = w + 1; si[i >= sx - 1 - w] = sx - 1 - w - 1
    sj[j <= w] = w + 1; sj[j >= sy - 1 - w] = sy - 1 - w - 1
    if is3d:
        sk[k <= w] = w + 1; sk[k >= sz - 1 - w] = sz - 1 - w - 1
    return g[sk, sj, si]


def init_from_flags(flags, ignoreWalls=False):
    """LevelsetGrid::initFromFlags, levelset.cpp:231-238"""
    m = (flags & TypeFluid) != 0
    if ignoreWalls:
        m |= (flags & TypeObstacle) != 0
    return np.where(m, f32(-0.5), f32(0.5)).astype(f32)


def combine_grid_vel(vel, weight, comb, phi=None, narrowBand=0.0, thresh=0.0):
    """knCombineVels, plugin/flip.cpp:748-770; returns (vel, combineVel)"""
    vel, comb = np.array(vel, f32), np.array(comb, f32)
    sz, sy, sx = vel.shape[:3]
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    base = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(f32)
    for c in range(3):
        deep = np.zeros((sz, sy, sx), bool)
        if phi is not None:
            p = base.copy()
            p[:, (c + 1) % 3] += f32(0.5)
            p[:, (c + 2) % 3] += f32(0.5)
            deep = (interp_real(phi, p) < -f32(narrowBand)).reshape(sz, sy, sx)
        take = ~deep & (weight[..., c] > f32(thresh))
        comb[..., c] = np.where(take, vel[..., c], comb[..., c])
        vel[..., c] = np.where(take, f32(-1), f32(0))
    return vel, comb


# ---------------------------------------------------------------------------------------------------------------------------------
# the particle system
# ---------------------------------------------------------------------------------------------------------------------------------
class Channel(object):
    """one pdata channel: kind 'vec3' | 'real' | 'int'; source grid (None: new values are 0) and whether it is sampled as a MAC grid"""

    def __init__(self, kind, data, source=None, mac=False):
        self.kind, self.source, self.mac = kind, source, mac
        self.data = np.array(data, np.int32 if kind == "int" else f32)

    def init_new(self, pos):
        n = pos.shape[0]
        if self.source is None:
            return np.zeros((n, 3) if self.kind == "vec3" else n, self.data.dtype)
        if self.kind == "vec3":
            return interp_mac(self.source, pos) if self.mac else interp_vec(self.source, pos)
        return interp_real(self.source, pos)


class Parts(object):
    """BasicParticleSystem: pos, flag, channels and the delete bookkeeping (mDeletes, mDeleteChunk), particle.h:171-173"""

    def __init__(self, pos, flag, channels=(), deletes=0, chunk=0, allow_compress=False):
        # allow_compress: ParticleBase::mAllowCompress.  BasicParticleSystem's constructor clears it (particle.cpp:134-138), so
        # kill() only counts there and the one compress of a call is doCompress() at its end; True is ParticleSystem's default
        self.allow_compress = bool(allow_compress)
        self.pos = np.array(pos, f32).reshape(-1, 3)
        self.flag = np.array(flag, np.int32)
        self.channels = list(channels)
        self.deletes, self.chunk = int(deletes), int(chunk)
        self.compresses = 0

    def copy(self):
        return Parts(self.pos, self.flag, [Channel(c.kind, c.data, c.source, c.mac) for c in self.channels], self.deletes, self.chunk,
                     self.allow_compress)

    def size(self): return self.flag.shape[0]

    def _arrays(self): return [self.pos, self.flag] + [c.data for c in self.channels]

    def _set_arrays(self, arrs):
        self.pos, self.flag = arrs[0], arrs[1]
        for c, a in zip(self.channels, arrs[2:]):
            c.data = a

    def compress_serial(self):
        """ParticleSystem::compress, particle.h:614-633, literally"""
        arrs = self._arrays()
        flag = self.flag
        n = nr = flag.shape[0]
        for i in range(n):
            while flag[i] & PDELETE:
                nr -= 1
                for a in arrs:
                    a[i] = a[nr]
                flag[nr] = PINVALID
        self._set_arrays([a[:nr].copy() for a in arrs])
        self.deletes, self.chunk = 0, nr // DELETE_PART
        self.compresses += 1

    def compress_par(self):
        """the same as a plan: M kept particles; the k-th hole below M (ascending) takes the k-th kept slot at or above M (descending)"""
        alive = (self.flag & PDELETE) == 0
        M = int(alive.sum())
        holes = np.nonzero(~alive[:M])[0]
        fill = np.nonzero(alive[M:])[0][::-1] + M
        assert len(holes) == len(fill)
        out = []
        for a in self._arrays():
            b = a[:M].copy()
            b[holes] = a[fill]
            out.append(b)
        self._set_arrays(out)
        self.deletes, self.chunk = 0, M // DELETE_PART
        self.compresses += 1

    def state(self):
        """everything a test compares"""
        d = {"pos": self.pos.copy(), "flag": self.flag.copy(),
             "book": np.array([self.deletes, self.chunk, self.compresses], np.int64)}
        for q, c in enumerate(self.channels):
            d["ch%d" % q] = c.data.copy()
        return d


def surface_ls(is3d, radiusFactor):
    """SURFACE_LS, flip.cpp:198-209: double product narrowed to Real"""
    rf = float(f32(radiusFactor))
    return f32(-1.0 * float(f32((np.sqrt(3.) if is3d else np.sqrt(2.)) * (rf + .01))))


def classify(pos, phi, narrowBand, sls):
    """flip.cpp:216-227 for every particle: cell (flat index, -1 outside), class 0 kill / 1 surface / 2 normal"""
    sz, sy, sx = phi.shape
    with np.errstate(invalid="ignore"):
        p = pos.astype(np.int64)           # toVec3i: truncation
    inb = (p >= 0).all(axis=1) & (p[:, 0] < sx) & (p[:, 1] < sy) & (p[:, 2] < sz)
    phiv = interp_real(phi, pos)
    nb = f32(narrowBand)
    kill = ~inb | (phiv > f32(0)) | ((nb > 0) & (phiv < -nb))
    cls = np.where(kill, 0, np.where(phiv > sls, 1, 2))
    cell = np.where(inb, p[:, 0] + sx * (p[:, 1] + sy * p[:, 2]), -1)
    return cell, cls


def _loop_serial(parts, cell, cls, ncell, maxp):
    """flip.cpp:214-237 with kill(), particle.h:423-427, literally: the particle identities travel with compress"""
    ident = Channel("int", np.arange(parts.size()))
    parts.channels.append(ident)
    tmp = np.zeros(ncell, np.int64)
    idx = 0
    while idx < parts.size():
        if not (parts.flag[idx] & PDELETE):
            p = ident.data[idx]
            kill = False
            if cls[p] == 0:
                kill = True
            else:
                num = tmp[cell[p]]
                if num > maxp and cls[p] == 2:
                    kill = True
                else:
                    tmp[cell[p]] = num + 1
            if kill:
                parts.flag[idx] |= PDELETE
                parts.deletes += 1
                if parts.deletes > parts.chunk and parts.allow_compress:
                    parts.compress_serial()
        idx += 1
    parts.channels.remove(ident)
    return tmp


def _loop_segmented(parts, cell, cls, ncell, maxp):
    """the order-free statement: rounds of classify / stable per-cell rank / prefix of kills / compress plan"""
    ident = Channel("int", np.arange(parts.size()))
    parts.channels.append(ident)
    tmp = np.zeros(ncell, np.int64)
    i0 = 0
    rounds = 0
    while i0 < parts.size():
        rounds += 1
        n = parts.size()
        sel = np.arange(i0, n)
        act = (parts.flag[sel] & PDELETE) == 0
        p = ident.data[sel]
        c, k = cell[p], cls[p]
        counted = act & (k != 0)
        order = np.lexsort((sel, np.where(counted, c, ncell)))
        cs = np.where(counted, c, ncell)[order]
        cnt = counted[order].astype(np.int64)
        run = np.cumsum(cnt) - cnt
        start = np.r_[True, cs[1:] != cs[:-1]]
        base = np.maximum.accumulate(np.where(start, run, 0))
        before = np.zeros(len(sel), np.int64)
        before[order] = run - base
        f = tmp[np.where(counted, c, 0)] + before
        kill = act & ((k == 0) | ((k == 2) & (f > maxp)))
        pre = parts.deletes + np.cumsum(kill)
        hit = np.nonzero(kill & (pre > parts.chunk))[0] if parts.allow_compress else []
        upto = len(sel) if len(hit) == 0 else hit[0] + 1
        kk = kill[:upto]
        parts.flag[sel[:upto][kk]] |= PDELETE
        kept = counted[:upto] & ~kk
        np.add.at(tmp, c[:upto][kept], 1)
        if len(hit) == 0:
            parts.deletes += int(kill.sum())
            break
        parts.compress_par()
        i0 = int(sel[hit[0]]) + 1
    parts.channels.remove(ident)
    parts.rounds = rounds
    return tmp


def mt_reals(n, seed=9832):
    """RandomStream(seed).getReal() n times: MT19937 with init_genrand seeding, float(randInt() * (1/4294967295))"""
    bg = np.random.MT19937()
    bg._legacy_seeding(int(seed))
    return (bg.random_raw(n).astype(np.float64) * (1.0 / 4294967295.0)).astype(f32)


def adjust_number(parts, flags, phi, minParticles, maxParticles, radiusFactor=1., narrowBand=-1., exclude=None, segmented=False):
    """adjustNumber, plugin/flip.cpp:204-262, in place on `parts`; returns the per-cell counts.  segmented: the order-free form"""
    sz, sy, sx = phi.shape
    is3d = sz > 1
    sls = surface_ls(is3d, radiusFactor)
    nb = f32(narrowBand)
    cell, cls = classify(parts.pos, phi, nb, sls)
    tmp = (_loop_segmented if segmented else _loop_serial)(parts, cell, cls, sx * sy * sz, int(maxParticles))
    # seeding, flat index order (FOR_IJK: i fastest)
    ph, fl, cnt = phi.ravel(), flags.ravel(), tmp
    skip = ph > sls
    if nb > 0:
        skip |= ph < -nb
    if exclude is not None:
        skip |= exclude.ravel() < f32(0)
    need = np.where(~skip & ((fl & TypeFluid) != 0), np.maximum(int(minParticles) - cnt, 0), 0)
    total = int(need.sum())
    cells = np.repeat(np.arange(sx * sy * sz), need)
    ijk = np.stack([cells % sx, (cells // sx) % sy, cells // (sx * sy)], axis=1).astype(f32)
    new = (ijk + mt_reals(3 * total).reshape(-1, 3)).astype(f32)
    if not is3d:
        new[:, 2] = f32(0.5)
    # doCompress, particle.h:142-145
    if parts.deletes > parts.chunk:
        parts.compress_par() if segmented else parts.compress_serial()
    # insertBufferedParticles, particle.h:636-663
    parts.flag &= ~np.int32(PNEW)
    if total:
        for ch in parts.channels:
            ch.data = np.concatenate([ch.data, ch.init_new(new).astype(ch.data.dtype)])
        parts.pos = np.concatenate([parts.pos, new])
        parts.flag = np.concatenate([parts.flag, np.full(total, PNEW, np.int32)])
    parts.inserted = total
    return tmp.reshape(sz, sy, sx)


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def smooth_field(dims, rng, amp=1.0):
    sx, sy, sz = dims
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    a = rng.uniform(0.2, 0.6, 3)
    ph = rng.uniform(0, 6, 3)
    return (amp * (np.sin(a[0] * i + ph[0]) + np.sin(a[1] * j + ph[1]) + (np.sin(a[2] * k + ph[2]) if sz > 1 else 0))).astype(f32)


def adjust_inputs(dims, seed, max_per_cell=14, deleted_frac=0.05, outside=12, pool_height=0.55, air=2.0, dense_frac=0.15):
    """a liquid pool with a wavy surface: flags, phi, exclude (an obstacle levelset), a MAC grid, a Real grid; particles 0..max_per_cell
    per cell in shuffled index order, some PDELETE already, some outside the domain on both sides; channels Vec3 (MAC source), Real
    (source), Real (none), Int"""
    sx, sy, sz = dims
    rng = np.random.RandomState(seed)
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    phi = ((j + 0.5) - pool_height * sy + 0.8 * smooth_field(dims, rng)).astype(f32)
    flags = np.where(phi <= 0, TypeFluid, TypeEmpty).astype(np.int32)
    wall = (i == 0) | (i == sx - 1) | (j == 0) | (j == sy - 1)
    if sz > 1:
        wall |= (k == 0) | (k == sz - 1)
    flags[wall] = TypeObstacle
    c = np.array([0.3 * sx, 0.2 * sy, 0.5 * sz])
    excl = (np.sqrt((i + 0.5 - c[0]) ** 2 + (j + 0.5 - c[1]) ** 2 + ((k + 0.5 - c[2]) ** 2 if sz > 1 else 0)) - 0.2 * sy).astype(f32)
    vel = np.stack([smooth_field(dims, rng, 0.5) for _ in range(3)], axis=-1).astype(f32)
    if sz == 1:
        vel[..., 2] = 0
    real = smooth_field(dims, rng, 2.0)
    ncells = sx * sy * sz
    n_cell = np.where(rng.rand(ncells) < dense_frac, rng.randint(0, max_per_cell + 1, ncells), rng.randint(0, min(4, max_per_cell + 1), ncells))
    n_cell[phi.ravel() > air] = 0                      # no particles far in the air; some above the surface stay
    cells = np.repeat(np.arange(sx * sy * sz), n_cell)
    ijk = np.stack([cells % sx, (cells // sx) % sy, cells // (sx * sy)], axis=1)
    pos = (ijk + rng.randint(1, 1024, ijk.shape) / 1024.).astype(f32)       # few mantissa bits: the fixture stays small
    if sz == 1:
        pos[:, 2] = f32(0.5)
    if outside:
        out = rng.uniform(-3, 0, (outside, 3)).astype(f32)
        out[outside // 2:] = (np.array(dims) + rng.uniform(0, 3, (outside - outside // 2, 3))).astype(f32)
        if sz == 1:
            out[:, 2] = f32(0.5)
            out[::3, 2] = f32(1.25)
        pos = np.concatenate([pos, out])
    pos = pos[rng.permutation(pos.shape[0])]
    n = pos.shape[0]
    flag = np.where(rng.rand(n) < deleted_frac, PDELETE, 0).astype(np.int32) | rng.randint(0, 2, n).astype(np.int32)
    q = lambda *shape: rng.randint(-64, 65, shape) / 64.
    chans = [Channel("vec3", q(n, 3), vel, True), Channel("real", q(n), real), Channel("real", q(n)), Channel("int", rng.randint(-5, 100, n))]
    return dict(flags=flags, phi=phi, exclude=excl, vel=vel, real=real, parts=Parts(pos, flag, chans))


# the per-call cases of the fixture: name -> (dims, seed, generator options, [(book or None, call arguments), ...]); a case with
# two calls runs the second on the output of the first
ADJUST_CASES = {
    # a fresh (0, 0) system: the first kill compresses
    "fresh3d": ((16, 12, 10), 11, {}, [((0, 0), dict(minParticles=4, maxParticles=8))]),
    "fresh2d": ((40, 30, 1), 12, {}, [((0, 0), dict(minParticles=2, maxParticles=4, narrowBand=3., exclude=True))]),
    # few kills under a large chunk: nothing compresses; the second call crosses the threshold mid-loop
    "two_calls": ((16, 12, 10), 13, dict(deleted_frac=0.0, outside=4, max_per_cell=6, air=0.2),
                  [((0, 400), dict(minParticles=2, maxParticles=20)),
                   (None, dict(minParticles=4, maxParticles=3, narrowBand=3., radiusFactor=1.5))]),
    # several compresses in one call
    "multi3d": ((16, 12, 10), 14, dict(deleted_frac=0.3), [((3, 40), dict(minParticles=8, maxParticles=2, narrowBand=3., exclude=True,
                                                                      radiusFactor=1.5))]),
    "multi2d": ((40, 30, 1), 15, dict(deleted_frac=0.1), [((0, 10), dict(minParticles=4, maxParticles=3, radiusFactor=1.5))]),
    # nothing killed, nothing seeded: only PNEW is cleared
    "noop": ((16, 12, 10), 16, dict(deleted_frac=0.0, outside=0, max_per_cell=3),
             [((0, 0), dict(minParticles=0, maxParticles=100))]),
}


# (case, allow_compress) pairs of the fixture: every case with compress allowed (ParticleSystem::kill's mid-loop compress), and
# the cases below as a BasicParticleSystem runs them in the reference (mAllowCompress false: kills counted, one compress at the end)
ADJUST_RUNS = [(n, True) for n in ADJUST_CASES] + [(n, False) for n in ("fresh3d", "fresh2d", "two_calls")]


def adjust_case(name, allow_compress=False):
    dims, seed, opt, calls = ADJUST_CASES[name]
    I = adjust_inputs(dims, seed, **opt)
    I["parts"].allow_compress = bool(allow_compress)
    if name == "noop":      # keep only particles the loop keeps: in the liquid, below the surface band or in it
        p = I["parts"]
        cell, cls = classify(p.pos, I["phi"], f32(-1), surface_ls(dims[2] > 1, 1.))
        keep = cls != 0
        p._set_arrays([a[keep] for a in p._arrays()])
    return I, calls


def run_adjust_case(name, allow_compress=False, segmented=False):
    """every call of a case on the model: list of state dicts (see Parts.state), with 'tmp' the per-cell counts"""
    I, calls = adjust_case(name, allow_compress)
    p = I["parts"]
    out = []
    for book, kw in calls:
        if book is not None:
            p.deletes, p.chunk = book
        p.compresses = 0
        kw = dict(kw)
        kw["exclude"] = I["exclude"] if kw.get("exclude") else None
        tmp = adjust_number(p, I["flags"], I["phi"], segmented=segmented, **kw)
        st = p.state()
        st["tmp"] = tmp.astype(np.int32)
        out.append(st)
    return out


def random_loop_case(rng):
    """the generator of the serial = segmented check: 1-400 particles, 1-30 cells, chunk from 0, n/20, n/10, n"""
    n = rng.randint(1, 400)
    ncell = rng.randint(1, 30)
    cell = rng.randint(0, ncell, n)
    cls = rng.choice(3, n, p=rng.dirichlet([1, 1, 3]))
    flag = (np.where(rng.rand(n) < rng.choice([0, 0.05, 0.3]), PDELETE, 0) | rng.randint(0, 2, n)).astype(np.int32)
    maxp = rng.randint(0, 10)
    md = rng.randint(0, 10)
    chunk = int(rng.choice([0, n // 20, n // 10, n]))
    return cell, cls, flag, ncell, maxp, md, chunk


def run_loop(cell, cls, flag, ncell, maxp, md, chunk, segmented, allow_compress=True):
    p = Parts(np.zeros((len(flag), 3), f32), flag, [Channel("int", np.arange(len(flag)))], md, chunk, allow_compress)
    tmp = (_loop_segmented if segmented else _loop_serial)(p, cell, cls, ncell, maxp)
    return p.flag, p.channels[0].data, tmp, p.deletes, p.chunk, p.compresses


COMBINE_CASES = {"c3d_phi": ((14, 11, 9), 21, True, 2.0, 0.0), "c3d_nophi": ((14, 11, 9), 22, False, 0.0, 0.5),
                 "c2d_phi": ((20, 17, 1), 23, True, 2.0, 0.5), "c2d_nophi": ((20, 17, 1), 24, False, 0.0, 0.0)}


def combine_inputs(name):
    dims, seed, with_phi, nb, thresh = COMBINE_CASES[name]
    sx, sy, sz = dims
    rng = np.random.RandomState(seed)
    vel = rng.uniform(-1, 1, (sz, sy, sx, 3)).astype(f32)
    comb = rng.uniform(-1, 1, (sz, sy, sx, 3)).astype(f32)
    weight = np.where(rng.rand(sz, sy, sx, 3) < 0.4, 0, rng.uniform(0, 1.2, (sz, sy, sx, 3))).astype(f32)
    j = np.arange(sy).reshape(1, sy, 1)
    phi = ((j + 0.5) - 0.7 * sy + smooth_field(dims, rng)).astype(f32) if with_phi else None
    return dict(vel=vel, weight=weight, comb=comb, phi=phi, narrowBand=nb, thresh=thresh)


NEUMANN_DIMS = {"3d": (13, 11, 9), "2d": (15, 12, 1)}


def neumann_inputs(which, seed=31):
    sx, sy, sz = NEUMANN_DIMS[which]
    rng = np.random.RandomState(seed)
    return rng.uniform(-1, 1, (sz, sy, sx)).astype(f32), rng.uniform(-1, 1, (sz, sy, sx, 3)).astype(f32)


def flags_inputs(which, seed=41):
    sx, sy, sz = NEUMANN_DIMS[which]
    rng = np.random.RandomState(seed)
    return rng.choice([TypeFluid, TypeObstacle, TypeEmpty, TypeFluid | 64, TypeObstacle | 8, TypeEmpty | 16], (sz, sy, sx)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# bridges between a device particle system of the package and the model
# ---------------------------------------------------------------------------------------------------------------------------------
def parts_to_device(m, s, parts, I):
    """build the package's particle system + channels + source grids from model inputs; returns (pp, channels, grids)"""
    pp = s.create(m.BasicParticleSystem)
    pp.set_positions(parts.pos, parts.flag)
    pp.mDeletes, pp.mDeleteChunk, pp.mAllowCompress = parts.deletes, parts.chunk, parts.allow_compress
    vel = s.create(m.MACGrid); vel.from_numpy(I["vel"])
    real = s.create(m.RealGrid); real.from_numpy(I["real"])
    chans = []
    for ch in parts.channels:
        pd = pp.create({"vec3": m.PdataVec3, "real": m.PdataReal, "int": m.PdataInt}[ch.kind])
        pd.from_numpy(ch.data)
        if ch.source is not None:
            pd.setSource(vel if ch.kind == "vec3" else real, isMAC=ch.mac)
        chans.append(pd)
    return pp, chans, (vel, real)


def device_state(pp, chans, compresses=0):
    d = {"pos": pp.get_positions(), "flag": pp.get_flags(), "book": np.array([pp.mDeletes, pp.mDeleteChunk, compresses], np.int64)}
    for q, pd in enumerate(chans):
        d["ch%d" % q] = pd.to_numpy()
    return d


def model_from_device(pp, chans, sources):
    """copy a device particle system into the model (the chain tests); sources: per channel (numpy grid or None, isMAC)"""
    cs = []
    for pd, (src, mac) in zip(chans, sources):
        kind = "vec3" if pd._ncomp == 3 else ("int" if pd.to_numpy().dtype == np.int32 else "real")
        cs.append(Channel(kind, pd.to_numpy(), src, mac))
    return Parts(pp.get_positions(), pp.get_flags(), cs, pp.mDeletes, pp.mDeleteChunk, pp.mAllowCompress)


# ---------------------------------------------------------------------------------------------------------------------------------
# the narrow-band loops (GPU backend only), the plugin sequence of the reference's narrow-band regression scene
# ---------------------------------------------------------------------------------------------------------------------------------
LOOPS = {"loop3d": dict(res=24, dim=3, steps=8), "loop2d": dict(res=48, dim=2, steps=12)}
NARROW_BAND = 3


def nb_loop(m, res, dim, steps, narrowBand=NARROW_BAND, before_adjust=None, after_adjust=None):
    """a breaking dam with narrow-band FLIP: particles within `narrowBand` cells of the surface, an advected grid velocity below.
    narrowBand <= 0: the same loop as full FLIP (no band in adjustNumber, particle velocities everywhere).  Returns a dict of
    per-step particle counts and CG iterations and the final fields and particles."""
    gs = m.vec3(res, res, res if dim == 3 else 1)
    s = m.Solver(name="main", gridSize=gs, dim=dim)
    s.timestep = 0.9
    minParticles = 2 ** dim
    flags = s.create(m.FlagGrid)
    phiParts, phi, pressure = s.create(m.LevelsetGrid), s.create(m.LevelsetGrid), s.create(m.RealGrid)
    vel, velOld, velParts, mapWeights = (s.create(m.MACGrid) for _ in range(4))
    pp = s.create(m.BasicParticleSystem)
    pVel = pp.create(m.PdataVec3)
    pindex, gpi = s.create(m.ParticleIndexSystem), s.create(m.IntGrid)
    flags.initDomain(boundaryWidth=0)
    phi.initFromFlags(flags)
    basin = s.create(m.Box, p0=gs * m.vec3(0, 0, 0), p1=gs * m.vec3(1.0, 0.15, 1.0))
    phi.join(basin.computeLevelset())
    dam = s.create(m.Box, p0=gs * m.vec3(0, 0.15, 0), p1=gs * m.vec3(0.4, 0.5, 0.8))
    phi.join(dam.computeLevelset())
    flags.updateFromLevelset(phi)
    m.sampleLevelsetWithParticles(phi=phi, flags=flags, parts=pp, discretization=2, randomness=0.4)
    m.mapGridToPartsVec3(source=vel, parts=pp, target=pVel)
    counts, iters = [], []
    band = narrowBand > 0
    for t in range(steps):
        pp.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4, deleteInObstacle=False)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=phi, order=1)
        flags.updateFromLevelset(phi)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2, clampMode=1)
        m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
        m.unionParticleLevelset(pp, pindex, flags, gpi, phiParts, radiusFactor=1)
        phi.addConst(1.)
        phi.join(phiParts)
        m.extrapolateLsSimple(phi=phi, distance=(narrowBand if band else NARROW_BAND) + 2, inside=True)
        m.extrapolateLsSimple(phi=phi, distance=3)
        flags.updateFromLevelset(phi)
        m.mapPartsToMAC(vel=velParts, flags=flags, velOld=velOld, parts=pp, partVel=pVel, weight=mapWeights)
        m.extrapolateMACFromWeight(vel=velParts, distance=2, weight=mapWeights)
        if band:
            m.combineGridVel(vel=velParts, weight=mapWeights, combineVel=vel, phi=phi, narrowBand=narrowBand - 1, thresh=0)
        else:
            m.combineGridVel(vel=velParts, weight=mapWeights, combineVel=vel, thresh=0)
        velOld.copyFrom(vel)
        m.addGravity(flags=flags, vel=vel, gravity=(0, -0.003, 0))
        m.setWallBcs(flags=flags, vel=vel)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure, phi=phi)
        iters.append(int(m.lastCgStats()["iterations"]))
        m.setWallBcs(flags=flags, vel=vel)
        m.extrapolateMACSimple(flags=flags, vel=vel, distance=5)
        m.flipVelocityUpdate(vel=vel, velOld=velOld, flags=flags, parts=pp, partVel=pVel, flipRatio=0.95)
        pVel.setSource(vel, isMAC=True)
        if before_adjust:
            before_adjust(t, pp, pVel, flags, phi, vel)
        m.adjustNumber(parts=pp, vel=vel, flags=flags, minParticles=minParticles, maxParticles=2 * minParticles, phi=phi,
                       narrowBand=narrowBand if band else -1.)
        if after_adjust:
            after_adjust(t, pp, pVel)
        counts.append(pp.pySize())
        s.step()
    return dict(counts=np.array(counts, np.int64), iters=np.array(iters, np.int64), phi=phi.to_numpy(), vel=vel.to_numpy(),
                phiParts=phiParts.to_numpy(), velParts=velParts.to_numpy(), pos=pp.get_positions(), flag=pp.get_flags(),
                pvel=pVel.to_numpy(), solver=s, parts=pp)
