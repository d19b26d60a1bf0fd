"""numpy model of the surface-mesh extension (include/open/manta_hip_mesh.h): LevelsetGrid::createMesh
(levelset.cpp:330-415) both as the literal serial sweep and as the order-free owner / rank statement the kernels implement,
Mesh::computeVertexNormals, the node advection of Mesh::advectInGrid, scale / offset / rotate, and the fixture's seeded inputs.
Arithmetic is done in numpy float32 / float64 scalars at the reference's promotion points.  tests/golden/mesh.npz holds what the
reference gave for the cases below (tools/record_mesh.py); arrays of more than FULL_LIMIT elements are kept as SHA-256 digests."""
import hashlib
import os

import numpy as np

f32, f64 = np.float32, np.float64
FULL_LIMIT = 4096
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh.npz")
ISO = f32(1e-4)
INVALID = f32(-1000.0)

# ---- the cube: corner offsets (x, y, z), the corner pairs of the 12 edges ------------------------------------------------------
CORNER = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))
EDGE = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))

# The classic marching-cubes triangle table (Lorensen & Cline; Bourke, "Polygonising a scalar field"), one word per sign
# configuration, in order: the hex digits are the local edge numbers of the triangle corners, three per triangle; "-" is no triangle.
TRI_WORDS = """
- 083 019 183981 12a 08312a 92a029 2832a8a98 3b2 0b28b0 19023b 1b219b98b 3a1ba3 0a108a8ba 3903b9ba9 98aa8b 478 430734
019847 419471731 12a847 34730412a 92a902847 2a9297273794 8473b2 b47b24204 90184723b 47b94b9b2921 3a13ba784 1ba14b1047b4
47890b9bab03 47b4b99ba 954 954083 054150 854835315 12a954 30812a495 52a542402 2a5325354348 95423b 0b208b495 05401523b
21525828b485 a3ba13954 4950818a18ba 54050b5bab03 54858aa8b 978579 930953573 078017157 153357 978957a12 a12950530573
802825857a52 2a5253357 7957893b2 95797292027b 23b018178157 b21b17715 958857a13a3b 5705097b010aba0 ba0b03a50807570 ba57b5
a65 0835a6 9015a6 1831985a6 165261 165126308 965906026 598582526328 23ba65 b08b20a65 01923b5a6 5a61929b298b 63b653513
08b0b50515b6 3b6036065059 65969bb98 5a6478 43047365a 1905a6847 a65197173794 612651478 125526304347 847905065026
739794329596269 3b2784a65 5a647242027b 01947823b5a6 9219b294b7b45a6 8473b53515b6 51b5b610b7b404b 059065036b63847
65969b4797b9 a4964a 4a649a083 a01a60640 83181686461a 149124264 308129249264 024426 832824426 a49a64b23 08228b49a4a6
3b201606461a 64161a48121b8b1 964936913b63 8b1810b61914641 3b6360064 648b68 7a678a89a 0730a709a67a a671a7178180 a67a71173
126168189867 269291679093739 780706602 732672 23ba68a89867 20727b09767a9a7 1801781a767a23b b21b17a61671 896867916b63136
091b67 7807063b0b60 7b6 76b 308b76 019b76 819831b76 a126b7 12a3086b7 2902a96b7 6b72a3a83a98 723627 708760620 276237019
162186198876 a76a17137 a7617a187108 03707a0a96a7 76a7a88a9 684b86 36b306046 86b846901 946963931b36 6846b82a1
12a30b06b046 4b846b0292a9 a93a32943b36463 823842462 042462 190234246438 194142246 8138618466a1 a10a06604 4634386a3039a93
a946a4 49576b 083495b76 50154076b b76834354315 954a1276b 6b712a083495 76b54a42a402 348354325a52b76 723762549
954086062687 362376150540 628687218485158 954a16176137 16a176107870954 40a4a503a6a737a 76a7a854a48a 6956b9b89
36b063056095 0b805b01556b 6b3635531 12a95b9b8b56 0b306b09656912a b85b56805a52025 6b36352a3a53 589528562382 956960062
158180568382628 156216 13616a386569896 a10a06950560 03856a a56 b5a75b b5ab75830 5b75ab190 a75ab7981831 b12b71751
08312717572b 9759279022b7 75272b592328982 25a235375 820852875a25 9015a35373a2 982921872a25752 135375 087071175 903935537
987597 5845a8ab8 5045b05abb30 01984a8aba45 ab4a45b34941314 2512852b8458 04b0b345b2b151b 0250592b5458b85 9452b3
25a352345384 5a2524420 3a235a385458019 5a2524192942 845853351 045105 845853905035 945 4b749b9ab 0834979b79ab
1ab1b414074b 3143481a474bab4 4b79b492b912 9749b791b2b1083 b74b42240 b74b42834324 29a279237749 9a7974a27870207
37a3a274a1a040a 1a2874 491417713 491417081871 403743 487 9a8ab8 30939bb9a 01a0a88ab 31ab3a 12b1b99b8 30939b1292b9 02b80b
32b 23828aa89 9a2092 23828a0181a8 1a2 138918 091 038 -
"""
TRI_TABLE = tuple(tuple(int(ch, 16) for ch in w) if w != "-" else () for w in TRI_WORDS.split())
assert len(TRI_TABLE) == 256
NTRI = np.array([len(r) // 3 for r in TRI_TABLE], np.int64)


def _geom(e):
    """-> (axis, origin) of local edge e: the axis it runs along and the lower of its two corners"""
    ca, cb = CORNER[EDGE[e][0]], CORNER[EDGE[e][1]]
    axis = [q for q in range(3) if ca[q] != cb[q]][0]
    return axis, tuple(min(ca[q], cb[q]) for q in range(3))


EDGE_ID = {_geom(e): e for e in range(12)}


def sharers(e):
    """the (up to four) cells that share local edge e of a cell, in sweep order (k outer, j, i inner): [(cell offset (di, dj, dk), the
    edge's local number in that cell)]; the cell itself is one of them"""
    axis, o = _geom(e)
    p, q = [a for a in range(3) if a != axis]          # q is the more significant axis of the sweep
    out = []
    for dq in (1, 0):
        for dp in (1, 0):
            off, lo = [0, 0, 0], list(o)
            off[p], off[q] = o[p] - dp, o[q] - dq
            lo[p], lo[q] = dp, dq
            out.append((tuple(off), EDGE_ID[(axis, tuple(lo))]))
    return out


SHARERS = tuple(sharers(e) for e in range(12))


# ---- node values (shared by the two statements of the sweep: they differ in who owns an edge and in the numbering) -----------------
def gradient(phi, i, j, k):
    """getGradient, grid.h:556-572, on a 3-D grid: central differences without the 1/2, i and j clamped to [1, size - 2]; the x and y
    differences are taken in the plane k as given, and only the z difference clamps k"""
    sz, sy, sx = phi.shape
    i = max(min(i, sx - 2), 1)
    j = max(min(j, sy - 2), 1)
    gx, gy = phi[k, j, i + 1] - phi[k, j, i - 1], phi[k, j + 1, i] - phi[k, j - 1, i]
    k = max(min(k, sz - 2), 1)
    return (gx, gy, phi[k + 1, j, i] - phi[k - 1, j, i])


EPS2 = f32(1e-6) * f32(1e-6)


def get_normalized(v, cnt=None):
    """getNormalized, vectorbase.h:405-416, S = float: |v|^2 in fp32, the `== 1` test in double, 1. / sqrt in double rounded once"""
    l = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    assert l.dtype == f32
    if abs(f64(l) - 1.0) < f64(EPS2):
        _count(cnt, "norm_one")
        return v
    if l > EPS2:
        _count(cnt, "norm_scaled")
        fac = f32(1.0 / np.sqrt(f64(l)))
        return (v[0] * fac, v[1] * fac, v[2] * fac)
    _count(cnt, "norm_zero")
    return (f32(0), f32(0), f32(0))


def _count(cnt, key, n=1):
    if cnt is not None:
        cnt[key] = cnt.get(key, 0) + n


def node_of_edge(phi, i, j, k, e, cnt=None):
    """the node cell (i, j, k) computes for its local edge e, with its own orientation e1 -> e2 (levelset.cpp:376-389) -> pos, normal"""
    a, b = EDGE[e]
    ca, cb = CORNER[a], CORNER[b]
    va, vb = -phi[k + ca[2], j + ca[1], i + ca[0]], -phi[k + cb[2], j + cb[1], i + cb[0]]
    if va == ISO or vb == ISO:
        _count(cnt, "iso_exact")
    mu = (ISO - va) / (vb - va)
    assert mu.dtype == f32
    p1 = (f32(i + ca[0]), f32(j + ca[1]), f32(k + ca[2]))
    p2 = (f32(i + cb[0]), f32(j + cb[1]), f32(k + cb[2]))
    pos = tuple(p1[c] + (p2[c] - p1[c]) * mu + f32(0.5) for c in range(3))
    g1 = gradient(phi, i + ca[0], j + ca[1], k + ca[2])
    g2 = gradient(phi, i + cb[0], j + cb[1], k + cb[2])
    w1 = 1.0 - f64(mu)                                        # `* (1.0 - mu)`: a double factor, each product rounded once
    n = tuple(f32(f64(g1[c]) * w1) + g2[c] * mu for c in range(3))
    return pos, get_normalized(n, cnt)


def _pack(nodes, normals, tris):
    return {"pos": np.array(nodes, f32).reshape(-1, 3), "normal": np.array(normals, f32).reshape(-1, 3),
            "tris": np.array(tris, np.int32).reshape(-1, 3)}


def _check_grid(phi):
    assert phi.dtype == f32 and phi.ndim == 3
    if phi.shape[0] == 1:
        raise RuntimeError("Only 3D grids supported so far")
    assert min(phi.shape) >= 3, "getGradient reads outside a grid thinner than 3 cells"


# ---- the literal serial sweep, levelset.cpp:343-408 ------------------------------------------------------------------------------
def create_mesh_serial(phi, cnt=None):
    _check_grid(phi)
    sz, sy, sx = phi.shape
    edgeV = [np.zeros(phi.shape, np.int64) for _ in range(3)]       # edgeVX, edgeVY, edgeVZ
    nodes, normals, tris = [], [], []
    with np.errstate(all="ignore"):
        for k in range(sz - 1):
            for j in range(sy - 1):
                for i in range(sx - 1):
                    skip, cube = False, 0
                    for l, (ox, oy, oz) in enumerate(CORNER):
                        v = -phi[k + oz, j + oy, i + ox]
                        if -v <= INVALID:
                            skip = True
                        if v < ISO:
                            cube |= 1 << l
                    if skip or cube == 0 or cube == 255:
                        continue
                    tri_idx = [0] * 12
                    for e in range(12):
                        if ((cube >> EDGE[e][0]) & 1) == ((cube >> EDGE[e][1]) & 1):
                            continue
                        axis, o = _geom(e)
                        slot = (k + o[2], j + o[1], i + o[0])
                        if edgeV[axis][slot] == 0:
                            p, n = node_of_edge(phi, i, j, k, e, cnt)
                            nodes.append(p)
                            normals.append(n)
                            edgeV[axis][slot] = len(nodes)
                        tri_idx[e] = edgeV[axis][slot]
                    row = TRI_TABLE[cube]
                    for t in range(0, len(row), 3):
                        tris.append([tri_idx[row[t]] - 1, tri_idx[row[t + 1]] - 1, tri_idx[row[t + 2]] - 1])
    return _pack(nodes, normals, tris)


# ---- the order-free statement: classify, own, scan, emit ------------------------------------------------------
def classify(phi):
    """-> cube index per cell [sz-1][sy-1][sx-1] (0: inactive, which covers the patterns 0 and 255 and cells with an invalid corner),
    and the cells that are inactive because of an invalid corner"""
    sz, sy, sx = phi.shape
    cube = np.zeros((sz - 1, sy - 1, sx - 1), np.int64)
    invalid = np.zeros(cube.shape, bool)
    for l, (ox, oy, oz) in enumerate(CORNER):
        c = phi[oz:sz - 1 + oz, oy:sy - 1 + oy, ox:sx - 1 + ox]
        cube |= ((-c) < ISO).astype(np.int64) << l
        invalid |= c <= INVALID
    cube[invalid | (cube == 255)] = 0
    return cube, invalid


def _shifted(a, off, fill=False):
    """b[k, j, i] = a[k + dk, j + dj, i + di] where that cell exists, else fill"""
    di, dj, dk = off
    b = np.full(a.shape, fill, a.dtype)
    src, dst = [], []
    for d, n in ((dk, a.shape[0]), (dj, a.shape[1]), (di, a.shape[2])):
        lo, hi = max(0, -d), min(n, n - d)
        if lo >= hi:
            return b
        dst.append(slice(lo, hi))
        src.append(slice(lo + d, hi + d))
    b[tuple(dst)] = a[tuple(src)]
    return b


def owned_edges(cube, invalid=None, cnt=None):
    """-> [cz][cy][cx][12] bool: the crossed edges of an active cell that no earlier active cell shares"""
    act = cube != 0
    owned = np.zeros(cube.shape + (12,), bool)
    for e in range(12):
        crossed = act & (((cube >> EDGE[e][0]) & 1) != ((cube >> EDGE[e][1]) & 1))
        earlier = np.zeros(cube.shape, bool)
        passed = np.zeros(cube.shape, bool)
        for off, _ in SHARERS[e]:
            if off == (0, 0, 0):
                break
            earlier |= _shifted(act, off)
            if invalid is not None:
                passed |= _shifted(invalid, off)
        owned[..., e] = crossed & ~earlier
        _count(cnt, "owner_passed", int((owned[..., e] & passed).sum()))
    return owned


def create_mesh(phi, cnt=None):
    _check_grid(phi)
    cube, invalid = classify(phi)
    cz, cy, cx = cube.shape
    act = cube != 0
    owned = owned_edges(cube, invalid, cnt)
    nown = owned.sum(-1).ravel()
    noff = (np.cumsum(nown) - nown).reshape(cube.shape)            # exclusive scans in sweep order
    ntri = NTRI[cube].ravel()
    toff = (np.cumsum(ntri) - ntri).reshape(cube.shape)
    nodes, normals = [], []
    tris = np.zeros((int(ntri.sum()), 3), np.int32)
    with np.errstate(all="ignore"):
        for k, j, i in np.argwhere(act):
            for e in np.flatnonzero(owned[k, j, i]):
                p, n = node_of_edge(phi, int(i), int(j), int(k), int(e), cnt)
                nodes.append(p)
                normals.append(n)
            row = TRI_TABLE[cube[k, j, i]]
            ids = {}
            for e in set(row):
                for (di, dj, dk), le in SHARERS[e]:
                    ii, jj, kk = i + di, j + dj, k + dk
                    if 0 <= ii < cx and 0 <= jj < cy and 0 <= kk < cz and act[kk, jj, ii]:
                        ids[e] = noff[kk, jj, ii] + int(owned[kk, jj, ii, :le].sum())
                        assert owned[kk, jj, ii, le]
                        break
            for t in range(0, len(row), 3):
                tris[toff[k, j, i] + t // 3] = [ids[row[t]], ids[row[t + 1]], ids[row[t + 2]]]
    assert len(nodes) == int(nown.sum())
    return _pack(nodes, normals, tris)


# ---- Mesh::computeVertexNormals, mesh.cpp:604-622 --------------------------------------------------------------------------------
def vertex_normals(pos, tris):
    """the serial accumulation in triangle order; `nm * (1.0 / (l0 * l2))` is a double factor, each product rounded once.  A degenerate
    triangle gives 0 * inf = NaN in its three nodes, which normalize() then turns into the zero vector (NaN fails both comparisons)."""
    nrm = np.zeros((pos.shape[0], 3), f32)
    with np.errstate(all="ignore"):
        for c in tris:
            p0, p1, p2 = pos[c[0]], pos[c[1]], pos[c[2]]
            n0, n1, n2 = p0 - p1, p1 - p2, p2 - p0
            l0, l1, l2 = [v[0] * v[0] + v[1] * v[1] + v[2] * v[2] for v in (n0, n1, n2)]
            nm = np.array([n0[1] * n1[2] - n0[2] * n1[1], n0[2] * n1[0] - n0[0] * n1[2], n0[0] * n1[1] - n0[1] * n1[0]], f32)
            for node, d in ((c[0], l0 * l2), (c[1], l0 * l1), (c[2], l1 * l2)):
                nrm[node] = nrm[node] + (nm.astype(f64) * (1.0 / f64(d))).astype(f32)
        for v in nrm:
            l = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
            if abs(f64(l) - 1.0) < f64(EPS2):
                continue
            if l > EPS2:
                norm = f32(np.sqrt(f64(l)))
                v *= f32(1.0 / f64(norm))
            else:
                v[:] = 0
    return nrm


# ---- Mesh::advectInGrid, mesh.cpp:301-315 + util/integrator.h:26-78 --------------------------------------------------------------
NF_FIXED = 1
INT_EULER, INT_RK2, INT_RK4 = 0, 1, 2


def _tri8(r, base, Y, Z, t, s, f):
    a = (r[base] * t[0] + r[base + Y] * t[1]) * s[0] + (r[base + 1] * t[0] + r[base + 1 + Y] * t[1]) * s[1]
    b = (r[base + Z] * t[0] + r[base + Y + Z] * t[1]) * s[0] + (r[base + 1 + Z] * t[0] + r[base + 1 + Y + Z] * t[1]) * s[1]
    return a * f[0] + b * f[1]


def interpol_mac(dims, vel, pos):
    """MACGrid::getInterpolated, util/interpol.h:131-164; vel is [3][n] planes, pos [3][np] -> [3][np]"""
    import p2g_model
    sx, sy, sz = dims
    Y, Z = sx, (sx * sy if sz > 1 else 0)
    (bx, by, bz), bs, bt, bf = p2g_model.build_index(dims, pos, False)
    (hx, hy, hz), hs, ht, hf = p2g_model.build_index(dims, pos, True)
    out = np.zeros(pos.shape, f32)
    out[0] = _tri8(vel[0], (bz * sy + by) * sx + hx, Y, Z, bt, hs, bf)
    out[1] = _tri8(vel[1], (bz * sy + hy) * sx + bx, Y, Z, ht, bs, bf)
    out[2] = _tri8(vel[2], (hz * sy + by) * sx + bx, Y, Z, bt, bs, hf)
    return out


def _node_velocity(dims, vel, pos, nflags, dt):
    """KnAdvectMeshInGrid: u = 0 for NfFixed nodes and outside isInBounds(pos, 1), else getInterpolated(pos) * dt"""
    sx, sy, sz = dims
    ip = pos.astype(np.int32)                                  # toVec3i: truncation
    inb = (ip[0] >= 1) & (ip[1] >= 1) & (ip[0] < sx - 1) & (ip[1] < sy - 1)
    inb &= ((ip[2] >= 1) & (ip[2] < sz - 1)) if sz > 1 else (ip[2] == 0)
    live = inb & ((nflags & NF_FIXED) == 0)
    u = np.zeros(pos.shape, f32)
    if live.any():
        u[:, live] = interpol_mac(dims, vel, np.ascontiguousarray(pos[:, live])) * f32(dt)
    return u


def advect_nodes(dims, vel, pos, nflags, dt, mode):
    """pos [3][np] float32 -> the advected positions; vel is the MAC grid as [3][n]"""
    assert pos.dtype == f32 and vel.dtype == f32
    x0 = pos.copy()
    with np.errstate(all="ignore"):
        u = _node_velocity(dims, vel, x0, nflags, dt)
        if mode == INT_EULER:
            return x0 + u
        if mode == INT_RK2:
            u = _node_velocity(dims, vel, x0 + f32(0.5) * u, nflags, dt)
            return x0 + u
        assert mode == INT_RK4
        ut = u + u                                             # uTotal(u), then `uTotal += u` (integrator.h:55)
        u = _node_velocity(dims, vel, x0 + f32(0.5) * u, nflags, dt)
        ut = ut + f32(2) * u
        u = _node_velocity(dims, vel, x0 + f32(0.5) * u, nflags, dt)
        ut = ut + f32(2) * u
        u = _node_velocity(dims, vel, x0 + u, nflags, dt)
        return x0 + f32(1. / 6.) * (ut + u)


# ---- scale / offset / rotate, mesh.cpp:332-373 -----------------------------------------------------------------------------------
ROTATE_AXES = ((1, 2), (0, 2), (0, 1))          # thetas.x, .y, .z


def rotate(pos, thetas, scalars):
    """pos [3][np]; scalars[q] = (sin, cos) of thetas[q] as the C library's float functions give them; a zero angle is skipped"""
    pos = pos.copy()
    for q, (a, b) in enumerate(ROTATE_AXES):
        if f32(thetas[q]) == f32(0):
            continue
        s, c = f32(scalars[q][0]), f32(scalars[q][1])
        if (a, b) == (0, 2):
            s = -s
        fa, fb = pos[a].copy(), pos[b].copy()
        pos[a] = fa * c - fb * s
        pos[b] = fb * c + fa * s
    return pos


# ---- fixture plumbing ------------------------------------------------------------------------------------------------------------
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


def mesh_same_as_fixture(golden, key, mesh):
    """mesh: dict(pos, normal, tris).  Counts first (always kept in full), then the three arrays"""
    counts = np.array([mesh["pos"].shape[0], mesh["tris"].shape[0]], np.int64)
    if not np.array_equal(counts, golden[key + "/counts"]):
        return "%s: %s nodes / triangles, recorded %s" % (key, counts, golden[key + "/counts"])
    for k in ("pos", "normal", "tris"):
        msg = same_as_fixture(golden, "%s/%s" % (key, k), mesh[k])
        if msg:
            return msg
    return None


def put_mesh(out, key, mesh):
    out[key + "/counts"] = np.array([mesh["pos"].shape[0], mesh["tris"].shape[0]], np.int64)
    for k in ("pos", "normal", "tris"):
        put(out, "%s/%s" % (key, k), mesh[k])


# ---- the createMesh cases: name -> phi [z][y][x] float32 -------------------------------------------------------------------------
def _rs(*key):
    return np.random.RandomState(int(hashlib.sha256(repr(key).encode()).hexdigest()[:8], 16))


def config_phi(c):
    """3x3x3: the 8 corners of cell (0, 0, 0) have sign pattern c (bit l set: -phi < iso), the other 19 values are seeded"""
    r = _rs("cfg", c)
    phi = (r.uniform(0.1, 1.0, (3, 3, 3)) * r.choice([-1.0, 1.0], (3, 3, 3))).astype(f32)
    for l, (ox, oy, oz) in enumerate(CORNER):
        m = abs(phi[oz, oy, ox])
        phi[oz, oy, ox] = m if (c >> l) & 1 else -m
    return phi


def _noise(name, dims, amp=1.0):
    sx, sy, sz = dims
    return (_rs(name).uniform(-1.0, 1.0, (sz, sy, sx)) * amp).astype(f32)


def _smooth(name, dims):
    """a few waves plus a little noise: a sparse surface through a large grid"""
    sx, sy, sz = dims
    r = _rs(name)
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    a = np.zeros((sz, sy, sx))
    for _ in range(4):
        kx, ky, kz = r.uniform(0.1, 0.6, 3)
        a += np.sin(kx * x + ky * y + kz * z + r.uniform(0, 6.28))
    a += r.uniform(-0.2, 0.2, a.shape)
    return a.astype(f32)


def _sphere(dims):
    sx, sy, sz = dims
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    c = np.array([sx, sy, sz], f64) * 0.5
    return (np.sqrt((x + 0.5 - c[0]) ** 2 + (y + 0.5 - c[1]) ** 2 + (z + 0.5 - c[2]) ** 2) - 0.3 * min(dims)).astype(f32)


def _invalid(name, dims):
    """noise with a block of invalid-time cells: the cells around the block lose the owners of their shared edges"""
    phi = _noise(name, dims)
    sz, sy, sx = phi.shape
    phi[sz // 3:sz // 3 + 2, sy // 3:sy // 3 + 2, sx // 3:sx // 3 + 2] = INVALID
    phi[-2, 1, 1] = f32(-1000.5)
    return phi


def _iso_exact(name, dims):
    phi = _noise(name, dims)
    phi[1, 1, 1] = -ISO               # -phi == iso exactly: the bit is clear, mu is 0 or 1 on its edges
    phi[2, 2, 1] = -ISO
    return phi


def _alt_x(dims):
    sx, sy, sz = dims
    phi = np.empty((sz, sy, sx), f32)
    phi[:] = np.where(np.arange(sx) % 2 == 0, f32(0.25), f32(-0.75))[None, None, :]
    return phi


def _plane_x(dims):
    """phi = 0.5 (i - 2.25): the central difference along x is exactly 1, so both gradients are (1, 0, 0) and the blend has length 1"""
    sx, sy, sz = dims
    phi = np.empty((sz, sy, sx), f32)
    phi[:] = (0.5 * (np.arange(sx) - 2.25)).astype(f32)[None, None, :]
    return phi


CASES = {
    "invalid": lambda: _invalid("invalid", (7, 6, 5)),
    "iso": lambda: _iso_exact("iso", (5, 4, 4)),
    "altx": lambda: _alt_x((6, 3, 4)),
    "planex": lambda: _plane_x((6, 4, 3)),
    "pos": lambda: np.full((4, 3, 5), 0.5, f32),
    "neg": lambda: np.full((4, 3, 5), -0.5, f32),
    "noise": lambda: _noise("noise", (9, 8, 7)),
    "sphere": lambda: _sphere((33, 31, 29)),
    "row65": lambda: _noise("row65", (65, 3, 3)),
    "col70": lambda: _noise("col70", (3, 3, 70)),
    "rand33": lambda: _with_block(_smooth("rand33", (33, 31, 29))),
}
SERIAL_CASES = ("invalid", "iso", "altx", "planex", "pos", "neg", "noise", "row65", "col70")     # small enough for the literal sweep


def _with_block(phi):
    phi = phi.copy()
    phi[10:13, 8:12, 14:20] = INVALID
    return phi


def case_phi(name):
    if name.startswith("cfg"):
        return config_phi(int(name[3:]))
    return CASES[name]()


def all_cases():
    return ["cfg%03d" % c for c in range(256)] + list(CASES)


_MODEL_CACHE = {}


def model_mesh(name):
    """the order-free model's mesh of a case, computed once per process; callers do not modify it"""
    if name not in _MODEL_CACHE:
        cnt = {}
        _MODEL_CACHE[name] = (create_mesh(case_phi(name), cnt), cnt)
    return _MODEL_CACHE[name]


# ---- advection / transform cases -------------------------------------------------------------------------------------------------
ADV_DIMS = (12, 10, 9)
ADV_DT = 0.75
ADV_SIZES = (0, 1, 63, 64, 65, 5000)


def advect_inputs(n):
    """-> vel [3][cells], pos [3][n], node flags [n]: some nodes fixed, some outside isInBounds(pos, 1), some beside the domain"""
    sx, sy, sz = ADV_DIMS
    r = _rs("adv", n)
    vel = r.uniform(-1.5, 1.5, (3, sx * sy * sz)).astype(f32)
    pos = (r.uniform(-1.0, 1.0, (3, n)) * 0.5 + 0.5) * np.array([[sx], [sy], [sz]]) * 1.1 - 0.3
    pos = pos.astype(f32)
    nflags = np.where(r.uniform(size=n) < 0.2, NF_FIXED, 0).astype(np.int32) | np.where(r.uniform(size=n) < 0.2, 2, 0).astype(np.int32)
    return vel, pos, nflags


ROT_THETAS = ((0.3, -1.1, 2.5), (0.0, 0.7, 0.0), (3.14159265, 0.0, -0.001), (0.0, 0.0, 0.0))
XF_SCALE, XF_OFFSET = (1.5, -0.25, 3.0), (0.1, -7.0, 2.5)


def xf_inputs(n=200):
    return (_rs("xf", n).uniform(-4.0, 20.0, (n, 3))).astype(f32)


# ---- computeVertexNormals cases --------------------------------------------------------------------------------------------------
VNORM_CASES = ("noise", "fan", "degenerate")


def vnorm_inputs(name):
    """-> pos [n][3], tris [t][3].  fan: one node shared by 12 triangles; degenerate: a triangle with a repeated node (0 * inf = NaN
    in its nodes), one with three equal nodes and one of three collinear nodes (a zero contribution)"""
    if name == "noise":
        m = model_mesh("noise")[0]
        return m["pos"], m["tris"]
    r = _rs("vnorm", name)
    if name == "fan":
        a = np.linspace(0, 2 * np.pi, 13)[:12]
        ring = np.stack([np.cos(a), np.sin(a), r.uniform(-0.3, 0.3, 12)], 1) * r.uniform(0.5, 1.5, (12, 1))
        pos = np.concatenate([[[0.1, -0.2, 0.4]], ring]).astype(f32)
        tris = np.array([[0, 1 + i, 1 + (i + 1) % 12] for i in range(12)], np.int32)
        return pos, tris
    pos = r.uniform(-1, 1, (8, 3)).astype(f32)
    pos[6] = pos[5] + (pos[5] - pos[4])              # 4, 5, 6 collinear
    tris = np.array([[0, 1, 2], [1, 1, 3], [2, 3, 4], [7, 7, 7], [4, 5, 6], [0, 2, 5]], np.int32)
    return pos, tris


SAVE_CASE, SAVE_DIMS = "iso", (5, 4, 4)

# ---- the recorded FLIP loop (tests/test_gpu_mesh.py; tools/mesh_record.cpp: rec_loop_mesh) ------------------------------------------
LOOP_RES, LOOP_STEPS, LOOP_ADV_STEPS = 32, 8, 3
