"""numpy statement of the array bridge and the MLFLIP data plugins (include/open/manta_hip_mlflip.h; reference plugin/numpyconvert.cpp,
plugin/tfplugins.cpp), and the seeded inputs of the cases that tests/golden/mlflip.npz holds the reference's outputs of (the inputs are
regenerated here, never stored).

Layouts: a grid is [z][y][x] (int32 or float32), a vector grid [z][y][x][3], particle positions [np][3].  Everything is order-free: the
region labelling is stated as "the rank of the component's lowest flat index", not as a flood fill; flood_fill_regions below is the
literal serial algorithm of the reference, for the test that holds one against the other.
"""
import numpy as np

import mesh_model
import p2g_model

f32, f64, i32 = np.float32, np.float64, np.int32
PDELETE = 1 << 10
FLUID, OBSTACLE, EMPTY = 1, 2, 4


# ---- the copies, numpyconvert.cpp:29-223 -------------------------------------------------------------------------------------------
def convert(a, dtype):
    """the C conversion of an assignment: float -> int truncates towards zero, double -> float and int -> float round to nearest"""
    a = np.asarray(a)
    if np.issubdtype(a.dtype, np.floating) and np.issubdtype(np.dtype(dtype), np.integer):
        return np.trunc(a).astype(dtype)
    return a.astype(dtype)


def array_to_grid(arr, dims, kind):
    """kind "real" | "int" | "vec" -> the grid as [z][y][x](,[3])"""
    sx, sy, sz = dims
    shape = (sz, sy, sx, 3) if kind == "vec" else (sz, sy, sx)
    return convert(np.ascontiguousarray(arr).reshape(shape), i32 if kind == "int" else f32)


def grid_to_array(grid, dtype, shape=None):
    out = convert(grid, dtype)
    return out if shape is None else out.reshape(shape)


# ---- feature extraction, tfplugins.cpp:38-148 --------------------------------------------------------------------------------------
def stencil(window, is3d):
    """the stencil points in the order they are written: i outer, j, k inner; k = 0 only on a 2-D grid"""
    r = range(-window, window + 1)
    return np.array([(i, j, k) for i in r for j in r for k in (r if is3d else (0,))], i32).reshape(-1, 3)


def feature_width(kind, window, is3d):
    w = 2 * window + 1
    return w * w * (w if is3d else 1) * ((3 if is3d else 2) if kind == "vel" else 1)


def extract_feature(kind, dims, grid, pos, pflag, ptype, exclude, window, scale, fv, N_row, off_begin):
    """kind "vel" (grid [z][y][x][3]) | "phi" (float32 [z][y][x]) | "geo" (int32 [z][y][x]); fv is float32 with at least np * N_row
    values and is returned as a changed copy.  Rows of deleted or excluded slots and the rest of every row keep their values."""
    sx, sy, sz = dims
    is3d = sz > 1
    fv = np.array(fv, f32).copy()
    flat = fv.reshape(-1)
    pts = stencil(window, is3d)
    D = (3 if is3d else 2) if kind == "vel" else 1
    assert off_begin >= 0 and off_begin + len(pts) * D <= N_row and flat.size >= pos.shape[0] * N_row and window >= 0
    live = (pflag & PDELETE) == 0
    if ptype is not None:
        live &= (ptype & exclude) == 0
    rows = np.nonzero(live)[0]
    if rows.size == 0:
        return fv
    scale = f32(scale)
    for s, off in enumerate(pts):
        p = (pos[rows] + off.astype(f32)).astype(f32)                       # Vec3 + Vec3 in fp32
        pt = np.ascontiguousarray(p.T)
        col = rows * N_row + off_begin + s * D
        if kind == "vel":
            planes = np.ascontiguousarray(grid.reshape(-1, 3).T)
            v = mesh_model.interpol_mac(dims, planes, pt)
            for c in range(D):
                flat[col + c] = v[c] * scale
        elif kind == "phi":
            Y, Z = sx, (sx * sy if is3d else 0)
            (bx, by, bz), bs, bt, bf = p2g_model.build_index(dims, pt, False)
            flat[col] = mesh_model._tri8(grid.reshape(-1), (bz * sy + by) * sx + bx, Y, Z, bt, bs, bf) * scale
        else:
            c = p.astype(i32)                                               # (int)pos: truncation
            assert geo_inside(dims, p).all(), "extractFeatureGeo: a sample position outside the grid (the plugin's precondition)"
            flat[col] = grid.reshape(-1)[c[:, 0].astype(np.int64) + sx * c[:, 1] + (sx * sy if is3d else 0) * c[:, 2]].astype(f32) * scale
    return fv


def geo_inside(dims, p):
    """does every position truncate to a cell of the grid?  (on a 2-D grid the z index is not used: strideZ is 0)"""
    sx, sy, sz = dims
    c = np.trunc(p.astype(f64))
    ok = (c[:, 0] >= 0) & (c[:, 0] < sx) & (c[:, 1] >= 0) & (c[:, 1] < sy)
    if sz > 1:
        ok &= (c[:, 2] >= 0) & (c[:, 2] < sz)
    return ok


def geo_precondition(dims, pos, window):
    p = np.concatenate([(pos + o.astype(f32)).astype(f32) for o in stencil(window, dims[2] > 1)])
    return bool(geo_inside(dims, p).all())


# ---- regions, tfplugins.cpp:155-220 ------------------------------------------------------------------------------------------------
def border_free(flags, ctype):
    """the precondition of getRegions: no ctype cell in the outermost layer (of x and y; of z as well on a 3-D grid)"""
    m = (flags & ctype) != 0
    sz = m.shape[0]
    edge = m[:, 0].any() or m[:, -1].any() or m[:, :, 0].any() or m[:, :, -1].any()
    if sz > 1:
        edge = edge or m[0].any() or m[-1].any()
    return not edge


def component_roots(flags, ctype):
    """[z][y][x] int64: the lowest flat index of the cell's face-connected component of flags & ctype cells, -1 outside.  Hooking
    (every edge lowers the larger root to the smaller) and pointer jumping until nothing moves: no order of visits enters."""
    m = ((flags & ctype) != 0)
    sz, sy, sx = m.shape
    n = m.size
    idx = np.arange(n, dtype=np.int64).reshape(m.shape)
    edges = []
    for ax, step in ((2, 1), (1, sx), (0, sx * sy)):
        if ax == 0 and sz == 1:
            continue
        hi = [slice(None)] * 3
        lo = [slice(None)] * 3
        hi[ax], lo[ax] = slice(1, None), slice(None, -1)
        both = m[tuple(hi)] & m[tuple(lo)]
        a = idx[tuple(hi)][both]
        edges.append(np.stack([a, a - step], 1))
    e = np.concatenate(edges) if edges else np.zeros((0, 2), np.int64)
    parent = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = parent[e[:, 0]], parent[e[:, 1]]
        d = ra != rb
        if not d.any():
            break
        np.minimum.at(parent, np.maximum(ra[d], rb[d]), np.minimum(ra[d], rb[d]))
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    return np.where(m, parent.reshape(m.shape), -1)


def regions(flags, ctype):
    """getRegions -> (r, count): components numbered from 1 in the order of their lowest flat index"""
    root = component_roots(flags, ctype)
    roots = np.unique(root[root >= 0])                   # sorted
    r = np.zeros(flags.shape, i32)
    inside = root >= 0
    r[inside] = (np.searchsorted(roots, root[inside]) + 1).astype(i32)
    return r, int(roots.size)


def regional_counts(flags, ctype):
    """getRegionalCounts: the size of the cell's component, 0 outside"""
    root = component_roots(flags, ctype)
    inside = root >= 0
    r = np.zeros(flags.shape, i32)
    if inside.any():
        cnt = np.bincount(root[inside], minlength=flags.size)
        r[inside] = cnt[root[inside]].astype(i32)
    return r


def flood_fill_regions(flags, ctype):
    """the reference's getRegions as written (tfplugins.cpp:155-176): FOR_IDX, a depth-first fill per unlabelled ctype cell with the
    neighbours tried in the order -x, +x, -y, +y, -z, +z on the flat index, unchecked -- the recursion as an explicit stack"""
    sz, sy, sx = flags.shape
    f = flags.reshape(-1)
    n = f.size
    r = np.zeros(n, i32)
    steps = [-1, 1, -sx, sx] + ([-sx * sy, sx * sy] if sz > 1 else [])
    count = 0
    for start in range(n):
        if (f[start] & ctype) and not r[start]:
            count += 1
            r[start] = count
            stack = [[start, 0]]
            while stack:
                top = stack[-1]
                if top[1] == len(steps):
                    stack.pop()
                    continue
                q = top[0] + steps[top[1]]
                top[1] += 1
                assert 0 <= q < n, "the fill leaves the array: a ctype cell in the outermost layer"
                if (f[q] & ctype) and not r[q]:
                    r[q] = count
                    stack.append([q, 0])
    return r.reshape(flags.shape), count


def extend_region(flags, region, exclude, depth):
    """extendRegion: per round, every cell without flags & exclude with a face neighbour inside the grid that has flags & region becomes
    exactly `region`; all cells of a round are decided from the flags before it"""
    f = np.array(flags, i32).copy()
    sz = f.shape[0]
    for _ in range(max(int(depth), 0)):
        hit = (f & region) != 0
        near = np.zeros(f.shape, bool)
        near[:, :, 1:] |= hit[:, :, :-1]
        near[:, :, :-1] |= hit[:, :, 1:]
        near[:, 1:] |= hit[:, :-1]
        near[:, :-1] |= hit[:, 1:]
        if sz > 1:
            near[1:] |= hit[:-1]
            near[:-1] |= hit[1:]
        f[near & ((f & exclude) == 0)] = region
    return f


def mark_small_regions(flags, rcnt, mark, exclude, th=1):
    f = np.array(flags, i32).copy()
    f[((f & exclude) == 0) & (rcnt <= th)] = mark
    return f


def simple_numpy_test(grid, arr, scale):
    """grid(i, j, k) += scale * arr[j * sx + i], the product and the sum in fp32"""
    sz, sy, sx = grid.shape
    plane = np.asarray(arr, f32).reshape(-1)[:sx * sy].reshape(sy, sx)
    return (grid + f32(scale) * plane[None]).astype(f32)


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.RandomState(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def clear_border(m):
    m = m.copy()
    m[:, 0] = m[:, -1] = False
    m[:, :, 0] = m[:, :, -1] = False
    if m.shape[0] > 1:
        m[0] = m[-1] = False
    return m


def random_flags(dims, fill, seed, ctype=FLUID, other=EMPTY):
    """ctype cells at about `fill` of the interior, the outermost layer obstacle, extra bits (64, 256) sprinkled on both kinds"""
    sx, sy, sz = dims
    rng = _rng(sx, sy, sz, int(fill * 100), seed)
    m = clear_border(rng.rand(sz, sy, sx) < fill)
    f = np.where(m, ctype, other).astype(i32)
    f |= np.where(rng.rand(sz, sy, sx) < 0.1, 64, 0).astype(i32)
    border = ~clear_border(np.ones((sz, sy, sx), bool))
    f[border] = OBSTACLE
    return f


REGION_CASES = {      # name: (dims, fill, seed)
    "r7x5x4": ((7, 5, 4), 0.55, 1),
    "r33_30": ((33, 31, 29), 0.30, 2),
    "r33_55": ((33, 31, 29), 0.55, 3),
    "r33_80": ((33, 31, 29), 0.80, 4),
    "r16": ((16, 16, 16), 0.45, 5),
    "r12x9": ((12, 9, 1), 0.55, 6),
    "r40x37": ((40, 37, 1), 0.60, 7),
    "r3x3": ((3, 3, 1), 1.0, 8),
    "rnone": ((9, 8, 7), 0.0, 9),
}
REGION_EXTEND = dict(region=EMPTY, exclude=OBSTACLE, depth=2)      # what extendRegion is recorded with, on the case's flags
REGION_MARK = dict(mark=EMPTY | 256, exclude=OBSTACLE | EMPTY, th=2)


def region_flags(name):
    dims, fill, seed = REGION_CASES[name]
    return random_flags(dims, fill, seed)


def smooth_fields(dims, seed):
    """a MAC grid [z][y][x][3], a level set and a flag grid with values that separate every corner weight"""
    sx, sy, sz = dims
    rng = _rng(sx, sy, sz, seed, 77)
    vel = (rng.rand(sz, sy, sx, 3).astype(f32) * f32(4) - f32(2)).astype(f32)
    phi = (rng.rand(sz, sy, sx).astype(f32) * f32(6) - f32(3)).astype(f32)
    flags = rng.choice(np.array([1, 2, 4, 1 | 64, 4 | 16, 2 | 256], i32), size=(sz, sy, sx)).astype(i32)
    return vel, phi, flags


def feature_particles(dims, n, window, seed):
    """positions whose whole stencil truncates inside the grid (the geo precondition), some of them hard against that limit and on cell
    centres and faces; flags with deleted slots; a ptype channel with bits 1, 2, 4"""
    sx, sy, sz = dims
    rng = _rng(sx, sy, sz, n, window, seed)
    lo = f32(window)
    hi = np.array([sx - window, sy - window, (sz - window) if sz > 1 else 1], f32)
    pos = (lo + rng.rand(n, 3).astype(f32) * (hi - lo - f32(1e-3))).astype(f32)
    if sz == 1:
        pos[:, 2] = f32(0.5)
    def last(h):
        """the largest position below h whose upper stencil point still rounds below h + window"""
        v = np.nextafter(f32(h), f32(0))
        while f32(v + f32(window)) >= f32(h + window):
            v = np.nextafter(v, f32(0))
        return v

    k = min(n, 6)
    if k:
        pos[:k, 0] = np.array([lo, last(hi[0]), lo + f32(0.5), lo + f32(1), hi[0] - f32(0.5), lo], f32)[:k]
        pos[:k, 1] = np.array([lo, lo + f32(0.5), last(hi[1]), lo, lo + f32(1), hi[1] - f32(0.5)], f32)[:k]
    pflag = np.where(rng.rand(n) < 0.15, PDELETE | 1, rng.randint(0, 4, n)).astype(i32)
    ptype = rng.choice(np.array([0, 1, 2, 4, 3, 6], i32), size=n).astype(i32)
    assert geo_precondition(dims, pos, window)
    return pos, pflag, ptype


FEATURE_CASES = {      # name: (dims, particles, window, exclude, use ptype, scale, off_begin, slack at the end of a row)
    "f3d_w0": ((12, 10, 8), 37, 0, 2, True, 1.0, 3, 2),
    "f3d_w1": ((12, 10, 8), 41, 1, 2, True, 0.75, 5, 4),
    "f3d_w2": ((13, 12, 11), 23, 2, 4, True, 1.5, 1, 3),
    "f3d_all": ((12, 10, 8), 29, 1, 0, False, 1.0, 0, 0),
    "f2d_w0": ((14, 11, 1), 31, 0, 2, True, 2.0, 2, 1),
    "f2d_w1": ((14, 11, 1), 43, 1, 1, True, 0.5, 4, 2),
    "f2d_w2": ((17, 15, 1), 19, 2, 2, False, 1.0, 0, 5),
}
FILL = f32(-777.25)      # what the untouched entries of a recorded feature matrix hold


def feature_inputs(name):
    dims, n, window, exclude, use_ptype, scale, off_begin, slack = FEATURE_CASES[name]
    vel, phi, flags = smooth_fields(dims, 11)
    pos, pflag, ptype = feature_particles(dims, n, window, 5)
    is3d = dims[2] > 1
    widths = [feature_width(k, window, is3d) for k in ("vel", "phi", "geo")]
    N_row = off_begin + sum(widths) + slack
    return dict(dims=dims, vel=vel, phi=phi, flags=flags, pos=pos, pflag=pflag, ptype=ptype if use_ptype else None, exclude=exclude,
                window=window, scale=scale, off_begin=off_begin, widths=widths, N_row=N_row, n=n)


def feature_matrix(I, extract=extract_feature):
    """the three plugins into one matrix, as save_features of manta_gendata.py does: velocity, then phi, then geo, side by side"""
    fv = np.full((I["n"], I["N_row"]), FILL, f32)
    off = I["off_begin"]
    for kind, grid, w in zip(("vel", "phi", "geo"), (I["vel"], I["phi"], I["flags"]), I["widths"]):
        fv = extract(kind, I["dims"], grid, I["pos"], I["pflag"], I["ptype"], I["exclude"], I["window"], I["scale"], fv, I["N_row"], off)
        off += w
    return fv


COPY_DIMS = (7, 5, 4)


def copy_inputs(dims=COPY_DIMS):
    """arrays whose values separate the conversions: 2**24 + 1 (int -> float rounds), 1 + 2**-30 (double -> float rounds), -1.7 and
    1.7 (float -> int truncates towards zero)"""
    sx, sy, sz = dims
    n = sx * sy * sz
    rng = _rng(n, 3)
    ai = rng.randint(-1000, 1000, n).astype(i32)
    ai[:4] = [2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 24 + 3, 7]
    ad = (rng.rand(n) * 20 - 10).astype(f64)
    ad[:6] = [1 + 2.0 ** -30, -1.7, 1.7, -0.999, 2.5, 1 + 2.0 ** -24 + 2.0 ** -40]
    af = ad.astype(f32)
    av = (rng.rand(n * 3) * 20 - 10).astype(f64)
    av[:3] = [1 + 2.0 ** -30, -1.7, 1 - 2.0 ** -26]
    shape = (sz, sy, sx)
    return dict(i=ai.reshape(shape), f=af.reshape(shape), d=ad.reshape(shape), vd=av.reshape(shape + (3,)), vf=av.astype(f32).reshape(shape + (3,)))


def same(a, b):
    """bit for bit: shape, dtype and every word (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the recorded loop -------------------------------------------------------------------------------------------------------------
LOOP = dict(res=32, steps=8, dt=0.5, th=8, window=1, scale_num=1, snaps=(4, 8), every=7, head=48)
FULL_LIMIT = 40000      # arrays of more elements are kept in the fixture as the SHA-256 of their bytes, under <key>#sha


def put(out, key, a):
    import hashlib
    a = np.ascontiguousarray(a)
    if a.size > FULL_LIMIT:
        out[key + "#sha"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8).copy()
        out[key + "#shape"] = np.array(a.shape, np.int64)
    else:
        out[key] = a


def same_as_fixture(golden, key, a):
    """None where `a` is the recorded array bit for bit (or has its digest), else a description"""
    import hashlib
    a = np.ascontiguousarray(a)
    if key in golden.files:
        want = golden[key]
        if same(a, want):
            return None
        if a.shape != want.shape or a.dtype != want.dtype:
            return "%s: %s %s where the fixture has %s %s" % (key, a.shape, a.dtype, want.shape, want.dtype)
        u = "u%d" % a.dtype.itemsize
        d = np.argwhere(a.view(u) != want.view(u))
        return "%s: %d of %d words differ, first at %s: %r where the fixture has %r" % (key, len(d), a.size, d[0], a[tuple(d[0])], want[tuple(d[0])])
    if tuple(golden[key + "#shape"]) != a.shape:
        return "%s: shape %s where the fixture has %s" % (key, a.shape, tuple(golden[key + "#shape"]))
    got = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)
    return None if np.array_equal(got, golden[key + "#sha"]) else "%s: the digest of the %d values differs from the recorded one" % (key, a.size)


def loop_row_width():
    w = 2 * LOOP["window"] + 1
    return 5 * w ** 3


def gendata_loop(m, target="numpy"):
    """the recorded loop in the package's API (GPU backend): flip01_simple.py's 3-D dam break and, after every step, the labelling and
    -- at the steps LOOP["snaps"] -- the feature matrix and the two particle-data copies of manta_gendata.py.  target "numpy": the
    arrays are numpy arrays; "device": tensors on the solver's device.  Returns counts [steps][4] (particles, regions, labelled cells,
    particles with a label) and per snap (fv [np][N_row], labels [np], pVel [np][3], positions [np][3])."""
    import torch
    C = LOOP
    res, steps = C["res"], C["steps"]
    gs = m.vec3(res, res, res)
    s = m.Solver(name="main", gridSize=gs, dim=3)
    s.timestep = C["dt"]
    flags, work, phi = s.create(m.FlagGrid), s.create(m.FlagGrid), s.create(m.LevelsetGrid)
    vel, velOld, pressure, tmpVec3 = s.create(m.MACGrid), s.create(m.MACGrid), s.create(m.RealGrid), s.create(m.VecGrid)
    r = s.create(m.IntGrid)
    pp = s.create(m.BasicParticleSystem)
    pVel, pT = pp.create(m.PdataVec3), pp.create(m.PdataInt)
    pindex, gpi = s.create(m.ParticleIndexSystem), s.create(m.IntGrid)
    flags.initDomain(boundaryWidth=0)
    fluidbox = m.Box(parent=s, p0=gs * m.vec3(0, 0, 0), p1=gs * m.vec3(0.4, 0.6, 1))
    phiInit = fluidbox.computeLevelset()
    flags.updateFromLevelset(phiInit)
    m.sampleFlagsWithParticles(flags=flags, parts=pp, discretization=2, randomness=0.2)
    window, N_row = C["window"], loop_row_width()
    nst = (2 * window + 1) ** 3
    fscale = float(f32(C["scale_num"]) / f32(res))
    counts = np.zeros((steps, 4), np.int64)
    snaps = {}

    def array(n, dtype):
        if target == "numpy":
            return np.full(n, -777.25 if dtype == f32 else -7, dtype)
        return torch.full((n,), -777.25 if dtype == f32 else -7, dtype=torch.float32 if dtype == f32 else torch.int32, device=s.device)

    def host(a):
        if target != "numpy":
            s.sync()
            a = a.cpu().numpy()
        return a

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
        n = pp.pySize()
        work.copyFrom(flags)
        pT.setConst(FLUID)
        regions_ = m.getRegions(r=r, flags=work, ctype=FLUID)
        labelled = int((r.to_numpy() > 0).sum())
        m.getRegionalCounts(r=r, flags=work, ctype=FLUID)
        m.markSmallRegions(flags=work, rcnt=r, mark=EMPTY, exclude=OBSTACLE, th=C["th"])
        m.setPartType(parts=pp, ptype=pT, mark=EMPTY, stype=FLUID, flags=work, cflag=EMPTY)
        m.extendRegion(flags=work, region=EMPTY, exclude=OBSTACLE, depth=1)
        m.setPartType(parts=pp, ptype=pT, mark=0, stype=FLUID, flags=work, cflag=FLUID)
        labels = array(n, i32)
        m.copyPdataToArrayInt(target=labels, source=pT)
        labels = host(labels)
        counts[t] = [n, regions_, labelled, int((labels != 0).sum())]
        if t + 1 in C["snaps"]:
            fv = array(n * N_row, f32)
            m.extractFeatureVel(fv=fv, N_row=N_row, off_begin=0, p=pp, vel=vel, scale=fscale, ptype=pT, exclude=FLUID, window=window)
            m.extractFeaturePhi(fv=fv, N_row=N_row, off_begin=3 * nst, p=pp, phi=phi, scale=1.0, ptype=pT, exclude=FLUID, window=window)
            m.extractFeatureGeo(fv=fv, N_row=N_row, off_begin=4 * nst, p=pp, flag=flags, scale=1.0, ptype=pT, exclude=FLUID, window=window)
            pv = array(3 * n, f32)
            m.copyPdataToArrayVec3(target=pv, source=pVel)
            snaps[t + 1] = (host(fv).reshape(n, N_row), labels, host(pv).reshape(n, 3), pp.get_positions())
        s.step()
    return counts, snaps


# ---- region patterns: masks [z][y][x] of ctype cells with the outermost layer clear ------------------------------------------------
def _ijk(dims):
    sx, sy, sz = dims
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    return i, j, k


def serpentine(dims):
    """a one-cell-wide path through the whole interior: rows 1, 3, 5 ... of the planes 1, 3, 5 ... (every plane of a 2-D grid), joined at
    alternating ends, the planes joined by one cell at alternating ends of the plane's path"""
    sx, sy, sz = dims
    m = np.zeros((sz, sy, sx), bool)
    if sx < 3 or sy < 3:
        return m
    plane = np.zeros((sy, sx), bool)
    rows = list(range(1, sy - 1, 2))
    for q, j in enumerate(rows):
        plane[j, 1:sx - 1] = True
        if q + 1 < len(rows):
            plane[j + 1, (sx - 2) if q % 2 == 0 else 1] = True
    start = (rows[0], 1)
    end = (rows[-1], (sx - 2) if (len(rows) - 1) % 2 == 0 else 1)
    if sz == 1:
        m[0] = plane
        return m
    planes = list(range(1, sz - 1, 2))
    for q, k in enumerate(planes):
        m[k] = plane
        if q + 1 < len(planes):
            m[k + 1][end if q % 2 == 0 else start] = True
    return m


def region_pattern(name, dims, seed=0):
    """-> (flags, ctype)"""
    sx, sy, sz = dims
    i, j, k = _ijk(dims)
    ctype = FLUID
    if name == "none":
        m = np.zeros((sz, sy, sx), bool)
    elif name == "full":
        m = np.ones((sz, sy, sx), bool)
    elif name == "checker":
        m = (i + j + k) % 2 == 0
    elif name == "serpentine":
        m = serpentine(dims)
    elif name == "comb":                    # teeth along y (and planes) that meet only in the last interior row (and plane)
        m = (i % 2 == 1) & ((k % 2 == 1) | (sz == 1))
        m |= (j == sy - 2) & ((k % 2 == 1) | (sz == 1))
        if sz > 1:
            m |= (j == sy - 2) & (i == sx - 2)      # ... and the planes only along the last column of that row
    elif name == "ushape":
        m = ((i == 1) | (i == sx - 2) | (j == sy - 2)) & ((k == 1) | (k == sz - 2) | (sz == 1))
        if sz > 1:
            m |= (k > 0) & (j == sy - 2) & (i == sx - 2)
    elif name == "diagonal":                # 2 x 2 (x 2) blocks that touch at edges and corners only
        m = (i // 2 + j // 2 + (k // 2 if sz > 1 else 0)) % 2 == 0
    elif name == "twobits":
        rng = _rng(sx, sy, sz, seed, 5)
        v = rng.choice(np.array([FLUID, EMPTY, OBSTACLE, FLUID | 64, EMPTY | 16, 8], i32), size=(sz, sy, sx)).astype(i32)
        border = ~clear_border(np.ones((sz, sy, sx), bool))
        v[border] = OBSTACLE
        return v, FLUID | EMPTY
    else:
        return random_flags(dims, float(name[4:]) / 100.0, seed + 31), FLUID        # "fill30", "fill55", "fill80"
    m = clear_border(m)
    flags = np.where(m, FLUID | 64, EMPTY).astype(i32)
    flags[~clear_border(np.ones((sz, sy, sx), bool))] = OBSTACLE
    return flags, ctype


REGION_PATTERNS = ("none", "full", "checker", "serpentine", "comb", "ushape", "diagonal", "twobits", "fill30", "fill55", "fill80")
