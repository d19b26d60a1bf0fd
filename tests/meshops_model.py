"""numpy statement of the mesh connectivity tables, smoothMesh and killSmallComponents (include/open/manta_hip_meshops.h, DESIGN.md
section 26): the reference's literal serial loops (mesh.cpp:123-141, 238-292, 401-508, plugin/meshplugins.cpp:36-104, 563-619) next to
the order-free forms the device uses, and the seeded case generators.  Inputs are regenerated, never stored; the reference's outputs
are in tests/golden/meshops.npz (tools/record_meshops.py).

A mesh is a dict: pos[n][3] f32, normal[n][3] f32, flags[n] i32, tris[t][3] i32, tflags[t] i32."""
import ctypes
import ctypes.util
import os

import numpy as np

import mesh_model as MM

f32, f64, i32 = np.float32, np.float64, np.int32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshops.npz")
NF_FIXED = 1
MSG_SINGLETON = "can't rebuild corners, index without an opposite"
MSG_NON_MANIFOLD = "killSmallComponents: non-manifold edge"
_rs = MM._rs


def mesh(pos, tris, flags=None, normal=None, tflags=None):
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, i32).reshape(-1, 3)
    n, t = pos.shape[0], tris.shape[0]
    return {"pos": pos, "normal": np.zeros((n, 3), f32) if normal is None else np.ascontiguousarray(normal, f32),
            "flags": np.zeros(n, i32) if flags is None else np.ascontiguousarray(flags, i32), "tris": tris,
            "tflags": np.zeros(t, i32) if tflags is None else np.ascontiguousarray(tflags, i32)}


def copy_mesh(m):
    return {k: v.copy() for k, v in m.items()}


# ---- 1. connectivity ---------------------------------------------------------------------------------------------------------------
def check_tris(who, tris, n):
    """the one divergence from the reference: a triangle with a repeated node (or a node outside the mesh) is refused by name"""
    for t, (a, b, c) in enumerate(tris.tolist()):
        if min(a, b, c) < 0 or max(a, b, c) >= n:
            raise RuntimeError("%s: triangle %d names a node outside the mesh's %d nodes" % (who, t, n))
    for t, (a, b, c) in enumerate(tris.tolist()):
        if a == b or b == c or a == c:
            raise RuntimeError("%s: triangle %d has a repeated node" % (who, t))


def corners_literal(tris):
    """Mesh::rebuildCorners, mesh.cpp:243-276, the literal forward search (quadratic); -> opposite, or the reference's error"""
    T = tris.shape[0]
    node = tris.reshape(-1).tolist()
    nxt = [3 * (c // 3) + (c % 3 + 1) % 3 for c in range(3 * T)]
    prv = [3 * (c // 3) + (c % 3 + 2) % 3 for c in range(3 * T)]
    opp = [-1] * (3 * T)
    for c in range(3 * T):
        n, p = node[nxt[c]], node[prv[c]]
        for c2 in range(c + 1, 3 * T):
            n2 = node[nxt[c2]]
            if n2 != n and n2 != p:
                continue
            p2 = node[prv[c2]]
            if p2 != n and p2 != p:
                continue
            opp[c], opp[c2] = c2, c
            break
        if opp[c] < 0:
            raise RuntimeError(MSG_SINGLETON)
    return np.array(opp, i32).reshape(-1)


def corners(tris):
    """order-free: corners grouped by the unordered (next, prev) pair, ascending corner number inside a group c_1 < ... < c_g:
    opposite[c_i] = c_{i+1} for i < g, opposite[c_g] = c_{g-1}; a group of one gets -1.  -> opposite, singles, groups with g >= 3"""
    T = tris.shape[0]
    if T == 0:
        return np.zeros(0, i32), 0, 0
    a, b = np.roll(tris, -1, 1).reshape(-1).astype(np.int64), np.roll(tris, -2, 1).reshape(-1).astype(np.int64)
    key = np.minimum(a, b) * (1 << 32) + np.maximum(a, b)
    order = np.argsort(key, kind="stable")
    k = key[order]
    head = np.r_[True, k[1:] != k[:-1]]
    tail = np.r_[k[1:] != k[:-1], True]
    opp = np.full(3 * T, -1, i32)
    nxt, prv = np.r_[order[1:], -1], np.r_[-1, order[:-1]]
    opp[order] = np.where(~tail, nxt, np.where(~head, prv, -1))
    size = np.diff(np.r_[np.nonzero(head)[0], 3 * T])
    return opp, int((size == 1).sum()), int((size >= 3).sum())


def ring_literal(tris, n):
    """Mesh::rebuildLookup, mesh.cpp:281-292: std::set per node, walked ascending -> (nodeOff, nodes, triOff, tris)"""
    nodes, tr = [set() for _ in range(n)], [set() for _ in range(n)]
    for t, tri in enumerate(tris.tolist()):
        for c in range(3):
            nodes[tri[c]].add(tri[(c + 1) % 3])
            nodes[tri[c]].add(tri[(c + 2) % 3])
            tr[tri[c]].add(t)
    return _csr(nodes) + _csr(tr)


def _csr(sets):
    off = np.zeros(len(sets) + 1, i32)
    off[1:] = np.cumsum([len(s) for s in sets])
    return off, np.array([v for s in sets for v in sorted(s)], i32).reshape(-1)


def ring(tris, n):
    """order-free: the (node, neighbour) pairs sorted, the first of each kept; the corners sorted by node"""
    T = tris.shape[0]
    node = np.repeat(tris.reshape(-1).astype(np.int64), 2)
    nb = np.stack([np.roll(tris, -1, 1).reshape(-1), np.roll(tris, -2, 1).reshape(-1)], 1).reshape(-1).astype(np.int64)
    pairs = np.unique(node * (1 << 32) + nb)
    pn = pairs >> 32
    nodeOff = np.searchsorted(pn, np.arange(n + 1)).astype(i32)
    cn = tris.reshape(-1)
    order = np.argsort(cn, kind="stable")
    triOff = np.searchsorted(cn[order], np.arange(n + 1)).astype(i32)
    return nodeOff, (pairs & 0xffffffff).astype(i32), triOff, (order // 3).astype(i32) if T else np.zeros(0, i32)


def connectivity(who, m):
    """what Mesh._connectivity leaves, or its refusal: -> dict(opposite, nodeOff, nodes, triOff, tris, singles, multi)"""
    n = m["pos"].shape[0]
    check_tris(who, m["tris"], n)
    opp, singles, multi = corners(m["tris"])
    if singles:
        raise RuntimeError(MSG_SINGLETON)
    r = ring(m["tris"], n)
    return {"opposite": opp, "nodeOff": r[0], "nodes": r[1], "triOff": r[2], "tris": r[3], "singles": singles, "multi": multi}


# ---- 2. smoothMesh -----------------------------------------------------------------------------------------------------------------
def norm3(e):
    """norm(), vectorbase.h:384-389, on rows of fp32 vectors"""
    l = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
    eps2 = f32(1e-6) * f32(1e-6)
    with np.errstate(invalid="ignore"):
        r = np.sqrt(l)
    r = np.where(np.abs(l.astype(f64) - 1.0) < f64(eps2), f32(1), r)
    return np.where(l <= eps2, f32(0), r).astype(f32)


def smooth_step_literal(pos, nodeOff, nodes, triOff, str_, minLength):
    """one pass of meshplugins.cpp:55-81 node by node -> temp (a node without a triangle keeps Vec3(), the origin)"""
    temp = np.zeros_like(pos)
    for p in range(pos.shape[0]):
        if triOff[p + 1] == triOff[p]:
            continue
        dx, total = np.zeros(3, f32), f32(0)
        for j in nodes[nodeOff[p]:nodeOff[p + 1]]:
            edge = pos[j] - pos[p]
            ln = norm3(edge[None])[0]
            if ln > minLength:
                dx = dx + (edge.astype(f64) * (1.0 / f64(ln))).astype(f32)
                total = f32(total + ln)
            else:
                total = f32(0)
                break
        temp[p] = pos[p]
        if total != 0:
            temp[p] = temp[p] + dx * f32(str_ / total)
    return temp


def smooth_step(pos, nodeOff, nodes, triOff, str_, minLength):
    """the same, all nodes at once: ring position k of every node that is still walking"""
    n = pos.shape[0]
    deg = np.diff(nodeOff)
    ref = np.diff(triOff) > 0
    dx, total, alive = np.zeros((n, 3), f32), np.zeros(n, f32), ref.copy()
    for k in range(int(deg.max()) if n else 0):
        idx = np.nonzero(alive & (deg > k))[0]
        if idx.size == 0:
            break
        edge = pos[nodes[nodeOff[idx] + k]] - pos[idx]
        ln = norm3(edge)
        ok = ln > minLength
        with np.errstate(divide="ignore", invalid="ignore"):
            step = (edge.astype(f64) * (1.0 / ln.astype(f64))[:, None]).astype(f32)
        dx[idx[ok]] = dx[idx[ok]] + step[ok]
        total[idx[ok]] = total[idx[ok]] + ln[ok]
        total[idx[~ok]] = 0
        alive[idx[~ok]] = False
    temp = pos.copy()
    nz = ref & (total != 0)
    temp[nz] = temp[nz] + dx[nz] * (f32(str_) / total[nz])[:, None]
    temp[~ref] = 0
    return temp


def volume_terms(pos, tris):
    """[t][4] fp64: cvol and the components of (p1 + p2 + p3) * (cvol / 4), mesh.cpp:129-135"""
    p = pos.astype(f64)[tris]                       # [t][corner][xyz]
    p1, p2, p3 = p[:, 0], p[:, 1], p[:, 2]
    cx = p1[:, 1] * p2[:, 2] - p1[:, 2] * p2[:, 1]
    cy = p1[:, 2] * p2[:, 0] - p1[:, 0] * p2[:, 2]
    cz = p1[:, 0] * p2[:, 1] - p1[:, 1] * p2[:, 0]
    cvol = (cx * p3[:, 0] + cy * p3[:, 1] + cz * p3[:, 2]) / 6.0
    return np.concatenate([cvol[:, None], ((p1 + p2) + p3) * (cvol / 4.0)[:, None]], 1)


def serial_sums(terms):
    """the reference's order: one triangle after the other"""
    s = np.zeros(4, f64)
    for row in terms:
        s = s + row
    return s


def pairwise_sums(terms):
    a = terms.copy()
    while a.shape[0] > 1:
        if a.shape[0] % 2:
            a = np.concatenate([a, np.zeros((1, 4), f64)])
        a = a[0::2] + a[1::2]
    return a[0] if a.shape[0] else np.zeros(4, f64)


def sum_bound(terms):
    """|S_a - S_b| <= 2 * gamma_{T-1} * sum|term| for two summation orders of the same T terms (each within gamma_{T-1} * sum|term|
    of the exact sum: Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)"""
    T = terms.shape[0]
    if T < 2:
        return np.zeros(4, f64)
    u = 2.0 ** -53
    return 2.0 * ((T - 1) * u / (1.0 - (T - 1) * u)) * np.abs(terms).sum(0)


_libm = None


def cbrtf(x):
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.cbrtf.restype, _libm.cbrtf.argtypes = ctypes.c_float, [ctypes.c_float]
    return f32(_libm.cbrtf(ctypes.c_float(float(x))))


def rescale_scalars(s0, s1):
    """computeCenterOfMass's return values from the sums, and beta = cbrt(Real / Real) (the float overload) -> origCM, newCM, beta"""
    with np.errstate(all="ignore"):
        cm = [(s[1:] / s[0] if s[0] != 0.0 else s[1:]).astype(f32) for s in (s0, s1)]
        beta = cbrtf(f32(s0[0]) / f32(s1[0]))
    return cm[0], cm[1], beta


def smooth_mesh(m, dt, strength, steps=1, minLength=1e-5, literal=False, sums=None, terms=None):
    """smoothMesh on a copy -> (mesh, the 2 x 4 sums).  `sums` replaces the serial sums (the recorder's end points of the bound); a list
    given as `terms` receives the volume terms before and after the steps"""
    conn = connectivity("smoothMesh", m)
    out = copy_mesh(m)
    str_ = min(f32(f32(dt) * f32(strength)), f32(1))
    minLength = f32(minLength)
    t0 = volume_terms(out["pos"], out["tris"])
    s0 = serial_sums(t0)
    free = (out["flags"] & NF_FIXED) == 0
    step = smooth_step_literal if literal else smooth_step
    for _ in range(steps):
        temp = step(out["pos"], conn["nodeOff"], conn["nodes"], conn["triOff"], str_, minLength)
        out["pos"][free] = temp[free]
    t1 = volume_terms(out["pos"], out["tris"])
    s1 = serial_sums(t1)
    if terms is not None:
        terms[:] = [t0, t1]
    if sums is not None:
        s0, s1 = sums
    o, n, beta = rescale_scalars(s0, s1)
    with np.errstate(all="ignore"):
        out["pos"][free] = o[None] + (out["pos"][free] - n[None]) * beta
    return out, np.stack([s0, s1])


# ---- 3. killSmallComponents ----------------------------------------------------------------------------------------------------------
def components_literal(opposite, T):
    """meshplugins.cpp:571-596: the stack walk -> comp (1-based), numEl"""
    comp, numEl, cur = [0] * T, [], 0
    opp = opposite.tolist()
    for i in range(T):
        if comp[i] == 0:
            cur += 1
            comp[i] = cur
            stack, cnt = [i], 1
            while stack:
                tri = stack.pop()
                for c in range(3):
                    op = opp[3 * tri + c]
                    if op < 0:
                        continue
                    nt = op // 3
                    if comp[nt] == 0:
                        comp[nt] = cur
                        stack.append(nt)
                        cnt += 1
            numEl.append(cnt)
    return comp, numEl


def components(opposite, T):
    """order-free: every triangle carries the smallest triangle of its component (union-find over t -- opposite // 3)"""
    parent = list(range(T))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for c, op in enumerate(opposite.tolist()):
        if op >= 0:
            a, b = find(c // 3), find(op // 3)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(t) for t in range(T)], np.int64)


def taint_mask(opposite, T, elements, literal=False):
    if literal:
        comp, numEl = components_literal(opposite, T)
        return np.array([numEl[c - 1] < elements for c in comp], bool).reshape(-1), len(numEl)
    lab = components(opposite, T)
    size = np.bincount(lab, minlength=max(T, 1))
    return (size[lab] < elements).reshape(-1), int((lab == np.arange(T)).sum())


def remove_tris_literal(tris, tflags, taint):
    """removeTri, mesh.cpp:401-448, over the tainted triangles in descending order: the then-last triangle moves into the hole"""
    tr, fl = tris.tolist(), tflags.tolist()
    for t in sorted(np.nonzero(taint)[0].tolist(), reverse=True):
        if t != len(tr) - 1:
            tr[t], fl[t] = tr[-1], fl[-1]
        tr.pop()
        fl.pop()
    return np.array(tr, i32).reshape(-1, 3), np.array(fl, i32).reshape(-1)


def tri_sources(taint):
    """order-free: -> src with new[h] = old[src[h]] for h < T - K.  below[q] = tainted triangles < q; the kept slot h that is tainted
    takes the end of the chain q <- T - (K - below[q]) from h through tainted positions"""
    T, K = taint.shape[0], int(taint.sum())
    below = np.cumsum(taint) - taint
    src = np.arange(T - K)
    for h in np.nonzero(taint[:T - K])[0].tolist():
        q = T - (K - below[h])
        while taint[q]:
            q = T - (K - below[q])
        src[h] = q
    return src


def deleted_nodes_literal(tris, taint, n):
    """meshplugins.cpp:598-608: first appearance, triangles ascending, corners 0..2"""
    seen, out = [False] * n, []
    for j in np.nonzero(taint)[0].tolist():
        for v in tris[j].tolist():
            if not seen[v]:
                seen[v] = True
                out.append(v)
    return out


def deleted_nodes(tris, taint, n):
    """order-free: per node the first tainted corner that names it; the list is the nodes in the order of that corner"""
    first = np.full(n, np.iinfo(np.int64).max, np.int64)
    c = np.nonzero(np.repeat(taint, 3))[0]
    np.minimum.at(first, tris.reshape(-1)[c], c)
    d = np.nonzero(first != np.iinfo(np.int64).max)[0]
    return d[np.argsort(first[d], kind="stable")].tolist()


def new_index_literal(deleted, n):
    """removeNodes, mesh.cpp:457-484, the literal two-cursor loop -> new_index[len(deleted)]"""
    newsize = n - len(deleted)
    new_index = [0] * len(deleted)
    for d in deleted:
        if d >= newsize:
            new_index[d - newsize] = -1
    di = ni = 0
    while ni < len(new_index):
        while ni < len(new_index) and new_index[ni] == -1:
            ni += 1
        if ni >= len(new_index):
            break
        while di < len(new_index) and deleted[di] >= newsize:
            di += 1
        new_index[ni] = deleted[di]
        ni += 1
        di += 1
    return new_index


def new_index(deleted, n):
    """order-free: the i-th node >= newsize that is not deleted moves to the i-th entry of the list that is < newsize"""
    d = np.array(deleted, np.int64).reshape(-1)
    newsize = n - d.size
    out = np.full(d.size, -1, np.int64)
    kept = np.ones(d.size, bool)
    kept[d[d >= newsize] - newsize] = False
    out[kept] = d[d < newsize]
    return out.tolist()


def kill_small_components(m, elements=10, literal=False):
    """killSmallComponents on a copy -> (mesh, stats) or the package's refusal.  stats: components, tris, nodes (deleted)"""
    conn = connectivity("killSmallComponents", m)
    if conn["multi"]:
        raise RuntimeError(MSG_NON_MANIFOLD)
    n, T = m["pos"].shape[0], m["tris"].shape[0]
    taint, ncomp = taint_mask(conn["opposite"], T, elements, literal)
    deleted = (deleted_nodes_literal if literal else deleted_nodes)(m["tris"], taint, n)
    isdel = np.zeros(n, bool)
    isdel[deleted] = True
    shared = np.unique(m["tris"][~taint].reshape(-1))
    shared = shared[isdel[shared]]
    if shared.size:
        raise RuntimeError("killSmallComponents: node %d is shared with a kept component" % shared[0])
    out = copy_mesh(m)
    if literal:
        out["tris"], out["tflags"] = remove_tris_literal(m["tris"], m["tflags"], taint)
    else:
        src = tri_sources(taint)
        out["tris"], out["tflags"] = m["tris"][src].copy(), m["tflags"][src].copy()
    ni = (new_index_literal if literal else new_index)(deleted, n)
    newsize = n - len(deleted)
    for i, j in enumerate(ni):
        if j != -1:
            for k in ("pos", "normal", "flags"):
                out[k][j] = out[k][newsize + i]
    for k in ("pos", "normal", "flags"):
        out[k] = out[k][:newsize].copy()
    hi = out["tris"] >= newsize
    out["tris"][hi] = np.array(ni, i32)[out["tris"][hi] - newsize]
    return out, {"components": ncomp, "tris": int(taint.sum()), "nodes": len(deleted)}


def kill_message(stats):
    return "Killed small components : %d nodes, %d tris deleted." % (stats["nodes"], stats["tris"])


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def bipyramid(n, seed=0, centre=(3.0, 4.0, 5.0)):
    """n equatorial nodes 0..n-1, apexes n and n + 1: n + 2 nodes, 2n triangles, apex valence n; positions jittered"""
    r = _rs("bipyramid", n, seed)
    a = 2 * np.pi * np.arange(n) / n
    pos = np.concatenate([np.stack([2.0 * np.cos(a), 2.0 * np.sin(a), np.zeros(n)], 1), [[0, 0, 1.5], [0, 0, -1.5]]])
    pos = pos + r.uniform(-0.05, 0.05, pos.shape) + np.array(centre)
    i = np.arange(n)
    j = (i + 1) % n
    tris = np.concatenate([np.stack([i, j, np.full(n, n)], 1), np.stack([j, i, np.full(n, n + 1)], 1)])
    return mesh(pos, tris)


def tetrahedron(seed=0, centre=(2.0, 2.0, 2.0)):
    r = _rs("tetra", seed)
    pos = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], f64) + r.uniform(-0.1, 0.1, (4, 3)) + np.array(centre)
    return mesh(pos, [[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])


def book3():
    """three pages on the edge (0, 1), wings 2, 3, 4, closed by six caps: no group of one, seven groups of three"""
    pos = _rs("book3").uniform(0, 4, (5, 3))
    return mesh(pos, [[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 2, 3], [0, 3, 4], [0, 4, 2], [1, 3, 2], [1, 4, 3], [1, 2, 4]])


def book4():
    """two tetrahedra that share the edge (0, 1): one group of four"""
    pos = _rs("book4").uniform(0, 4, (6, 3))
    return mesh(pos, [[0, 1, 2], [1, 0, 3], [0, 2, 3], [1, 3, 2], [0, 1, 4], [1, 0, 5], [0, 4, 5], [1, 5, 4]])


def strip(n=5):
    pos = np.stack([np.arange(n + 2) * 0.5, (np.arange(n + 2) % 2) * 1.0, np.zeros(n + 2)], 1)
    return mesh(pos, [[i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2] for i in range(n)])


def sphere(res=17):
    phi = MM._sphere((res, res, res))
    c = MM.create_mesh(phi)
    return mesh(c["pos"], c["tris"], normal=c["normal"])


def two_blobs(res=24):
    """a large and a very small sphere: createMesh gives two components, the small one below ten triangles"""
    z, y, x = np.meshgrid(np.arange(res), np.arange(res), np.arange(res), indexing="ij")
    big = np.sqrt((x + 0.5 - 10.0) ** 2 + (y + 0.5 - 12.0) ** 2 + (z + 0.5 - 12.0) ** 2) - 6.3
    small = np.sqrt((x - 20.0) ** 2 + (y - 12.0) ** 2 + (z - 12.0) ** 2) - 0.6
    return np.minimum(big, small).astype(f32)


def permuted(m, seed):
    """the triangle list shuffled and every triangle rotated: corner order no longer follows node order"""
    r = _rs("perm", seed)
    out = copy_mesh(m)
    T = m["tris"].shape[0]
    p = r.permutation(T)
    rot = r.randint(0, 3, T)
    out["tris"] = np.stack([np.roll(m["tris"][p[t]], rot[t]) for t in range(T)]).astype(i32).reshape(-1, 3)
    out["tflags"] = m["tflags"][p].copy()
    return out


def with_nodes(m, extra_pos, extra_flags):
    out = copy_mesh(m)
    k = len(extra_flags)
    out["pos"] = np.concatenate([m["pos"], np.array(extra_pos, f32).reshape(k, 3)])
    out["normal"] = np.concatenate([m["normal"], np.zeros((k, 3), f32)])
    out["flags"] = np.concatenate([m["flags"], np.array(extra_flags, i32)])
    return out


def join(parts, seed=None, tri_seed=None):
    """the disjoint union of meshes; `seed` renumbers the nodes by a seeded permutation (killed nodes interleaved with kept ones),
    `tri_seed` shuffles the triangle list (components interleaved).  Node and triangle flags are set to recognisable values."""
    pos = np.concatenate([p["pos"] for p in parts])
    off = np.cumsum([0] + [p["pos"].shape[0] for p in parts])
    tris = np.concatenate([p["tris"] + off[q] for q, p in enumerate(parts)])
    n, T = pos.shape[0], tris.shape[0]
    flags, tflags = (np.arange(n) * 16).astype(i32), (np.arange(T) % 3).astype(i32)
    normal = _rs("join-normal", n).uniform(-1, 1, (n, 3)).astype(f32)
    if seed is not None:
        perm = _rs("join", seed).permutation(n)              # old node v becomes perm[v]
        inv = np.argsort(perm)
        pos, normal, flags, tris = pos[inv], normal[inv], flags[inv], perm[tris]
    if tri_seed is not None:
        p = _rs("join-tris", tri_seed).permutation(T)
        tris, tflags = tris[p], tflags[p]
    return mesh(pos, tris, flags=flags, normal=normal, tflags=tflags)


CONNECTIVITY_CASES = {
    "tetra": tetrahedron, "octa": lambda: bipyramid(4), "bipyr3": lambda: bipyramid(3), "bipyr61": lambda: bipyramid(61),
    "bipyr62": lambda: bipyramid(62), "bipyr63": lambda: bipyramid(63), "bipyr300": lambda: bipyramid(300), "sphere17": sphere,
    "book3": book3, "book4": book4, "empty": lambda: mesh(np.zeros((0, 3)), np.zeros((0, 3))),
    "nodes_only": lambda: mesh(np.ones((5, 3)), np.zeros((0, 3))),
    "perm_bipyr63": lambda: permuted(bipyramid(63), 1), "perm_sphere17": lambda: permuted(sphere(), 2),
    "isolated": lambda: with_nodes(permuted(bipyramid(5), 3), [[1, 1, 1], [2, 2, 2]], [0, 0]),
}
REFUSED_CASES = {
    "single": (lambda: mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]]), MSG_SINGLETON),
    "strip": (strip, MSG_SINGLETON),
    "repeated": (lambda: mesh(tetrahedron()["pos"], [[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0], [1, 1, 2]]), "%s: triangle 4 has a repeated node"),
}


def _smooth_two():
    return join([bipyramid(7, 1), tetrahedron(1, (9.0, 2.0, 3.0))])


def _coincident():
    m = bipyramid(6, 2)
    m["pos"][1] = m["pos"][0]              # two coincident neighbours: every node that sees both ... the pair itself does not move
    return m


def _fixed():
    m = bipyramid(9, 3)
    m["flags"][[0, 9]] = NF_FIXED
    return m


# name -> (mesh, dt, strength, steps, minLength)
SMOOTH_CASES = {
    "steps0": lambda: (bipyramid(8, 4), 0.5, 0.6, 0, 1e-5),
    "steps1": lambda: (bipyramid(8, 4), 0.5, 0.6, 1, 1e-5),
    "steps3": lambda: (bipyramid(63, 5), 0.5, 0.6, 3, 1e-5),
    "apex300": lambda: (bipyramid(300, 6), 0.5, 0.6, 1, 1e-5),
    "clamp": lambda: (bipyramid(8, 4), 1.0, 7.0, 1, 1e-5),
    "fixed": lambda: (_fixed(), 0.5, 0.6, 2, 1e-5),
    "coincident": lambda: (_coincident(), 0.5, 0.6, 1, 1e-5),
    "isolated": lambda: (with_nodes(bipyramid(5, 7), [[1, 1, 1], [2, 3, 4]], [0, NF_FIXED]), 0.5, 0.6, 1, 1e-5),
    "minlength": lambda: (bipyramid(8, 4), 0.5, 0.6, 2, 100.0),
    "two": lambda: (_smooth_two(), 0.5, 0.6, 2, 1e-5),
    "sphere17": lambda: (permuted(sphere(), 4), 0.5, 0.6, 3, 1e-5),
}


def _parts():
    return [bipyramid(6, 10), tetrahedron(2, (9, 2, 3)), bipyramid(4, 11, (2, 9, 3)), tetrahedron(3, (9, 9, 3)), bipyramid(5, 12, (5, 5, 9))]


def _chained():
    """twelve triangles, the tetrahedron's at 1, 2, 5 and 9: the removal of 9 takes old 11, that of 5 old 10, that of 2 takes position
    9 -- old 11 again, a chained move -- and that of 1 takes old 8"""
    m = join([tetrahedron(4), bipyramid(4, 13, (9, 2, 3))])                 # triangles 0-3 and 4-11
    order = [4, 0, 1, 5, 6, 2, 7, 8, 9, 3, 10, 11]
    m["tris"], m["tflags"] = m["tris"][order], m["tflags"][order]
    return m


# name -> (mesh, elements): 12-triangle, 4-triangle, 8-triangle, 4-triangle and 10-triangle components
KILL_CASES = {
    "equal": lambda: (join(_parts()), 4),                     # elements == the smallest size: strict <, nothing killed
    "plus1": lambda: (join(_parts()), 5),                     # the two tetrahedra go (second and fourth component)
    "first": lambda: (join([tetrahedron(2)] + _parts()[:1]), 5),
    "last": lambda: (join(_parts()[:2]), 5),
    "all": lambda: (join(_parts()), 100),
    "none_default": lambda: (join([bipyramid(6, 10), bipyramid(5, 12, (5, 5, 9))]), 10),
    "default": lambda: (join(_parts()), 10),                  # below ten: the tetrahedra and the octahedron
    "interleaved": lambda: (join(_parts(), seed=1), 9),
    "shuffled": lambda: (join(_parts(), seed=2, tri_seed=3), 9),
    "chained": lambda: (_chained(), 5),
    "isolated": lambda: (with_nodes(join(_parts(), seed=4, tri_seed=5), [[1, 1, 1], [2, 2, 2], [3, 3, 3]], [7, 8, 9]), 9),
    "sphere17": lambda: (join([permuted(sphere(), 6), tetrahedron(7, (1, 1, 1))], seed=8, tri_seed=9), 10),
}


def _shared():
    m = join([bipyramid(6, 10), tetrahedron(2, (9, 2, 3))])
    m["tris"][m["tris"] == 9] = 3              # a node of the tetrahedron is a node of the bipyramid: the components stay apart (no shared edge)
    return m


KILL_REFUSED = {
    "shared": (lambda: (_shared(), 5), "killSmallComponents: node 3 is shared with a kept component"),
    "book3": (lambda: (book3(), 5), MSG_NON_MANIFOLD),
    "strip": (lambda: (strip(), 5), MSG_SINGLETON),
}


# ---- fixture plumbing (as tests/mesh_model.py) -----------------------------------------------------------------------------------------
put, same_as_fixture = MM.put, MM.same_as_fixture
MESH_KEYS = ("pos", "normal", "flags", "tris", "tflags")


def put_mesh(out, key, m):
    out[key + "/counts"] = np.array([m["pos"].shape[0], m["tris"].shape[0]], np.int64)
    for k in MESH_KEYS:
        put(out, "%s/%s" % (key, k), m[k])


def mesh_same_as_fixture(golden, key, m):
    counts = np.array([m["pos"].shape[0], m["tris"].shape[0]], np.int64)
    if not np.array_equal(counts, golden[key + "/counts"]):
        return "%s: %s nodes / triangles, recorded %s" % (key, counts, golden[key + "/counts"])
    for k in MESH_KEYS:
        msg = same_as_fixture(golden, "%s/%s" % (key, k), m[k])
        if msg:
            return msg
    return None
