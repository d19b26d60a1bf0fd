"""numpy model of mesh-to-level-set rasterisation (meshSDF, mesh.cpp:868-1005) with every stage separate and with counters:
sources (count / emit order of the reference's push_back loop), binning (_cIndex, stable by cell), gather (SDFKernel's summation order,
fp32 throughout, the weight as the fp64 exp of the fp32 argument rounded once), flood fill (the literal stack loop and the closure it
ends in), plus the element-wise statements of ApplyMeshToGrid and KnApplyDensity.  The fp32 / fp64 map is DESIGN.md section 17.

The case generators are seeded; tests/golden/meshsdf.npz holds what the reference computed for them (tools/record_meshsdf.py)."""
import functools
import hashlib
import os

import numpy as np

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshsdf.npz")
GOLD = os.path.dirname(GOLDEN)
FULL_LIMIT = 4096
EPS2 = f32(1e-6) * f32(1e-6)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


# ---- host scalars, mesh.cpp:870, 978-982 -------------------------------------------------------------------------------------------
def params(sigma, cutoff):
    sigma, cutoff = f32(sigma), f32(cutoff)
    if cutoff < 0:
        cutoff = f32(f32(2) * sigma)
    safe = f32(f64(cutoff) + np.sqrt(3.0) * 0.5)
    return {"sigma": sigma, "cutoff": cutoff, "safeRadius2": f32(safe * safe), "cutoff2": f32(cutoff * cutoff),
            "isigma2": f32(1.0 / f64(f32(sigma * sigma))), "intRadius": int(f64(cutoff) + 0.5)}


# ---- stage 1: sources ----------------------------------------------------------------------------------------------------------------
def norm3(v):
    """norm, vectorbase.h:385-389 (S = float)"""
    l = f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))
    if l <= EPS2:
        return f32(0)
    return f32(1) if abs(f64(l) - 1.) < f64(EPS2) else f32(np.sqrt(l))


def normalized(v):
    """getNormalized, vectorbase.h:405-416 (S = float): the three branches of mesh_cells.h"""
    l = f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))
    if abs(f64(l) - 1.) < f64(EPS2):
        return v.copy(), "norm_one"
    if l > EPS2:
        fac = f32(1. / np.sqrt(f64(l)))
        return (v * fac).astype(f32), "norm_scaled"
    return np.zeros(3, f32), "norm_zero"


def tri_plan(p):
    """mesh.cpp:886-919 -> big, iterA, iterB, pA, pB, branch"""
    ln = [norm3(p[(e + 1) % 3] - p[e]) for e in range(3)]
    big = sum(1 << e for e in range(3) if ln[e] > f32(0.75))
    if big == 0:
        return 0, 0, 0, 0, 0, "none"
    n0, n1, n2 = (int(f32(ln[1] * f32(0.75))), int(f32(ln[2] * f32(0.75))), int(f32(ln[0] * f32(0.75))))
    if not big & 1:
        r = (n1, n2, 0, 1, "branch01")
    elif not big & 2:
        r = (n2, n0, 1, 2, "branch12")
    else:
        r = (n0, n1, 2, 0, "branch20")
    assert r[0] <= 32767 and r[1] <= 32767, "precondition: a sample count that the reference's short does not hold"
    return (big,) + r


def sources(pos, tris, mult):
    """-> spos[n][3], snrm[n][3], counters, per-triangle counts"""
    pos, mult = np.asarray(pos, f32).reshape(-1, 3), np.asarray(mult, f32)
    out_p, out_n, per_tri = [], [], []
    cnt = {"none": 0, "branch01": 0, "branch12": 0, "branch20": 0, "skipped_w": 0, "iter_zero": 0, "norm_one": 0, "norm_scaled": 0,
           "norm_zero": 0}
    for t in np.asarray(tris, np.int32).reshape(-1, 3):
        p = pos[t]
        a, b = p[1] - p[0], p[2] - p[0]
        cr = np.array([f32(a[1] * b[2]) - f32(a[2] * b[1]), f32(a[2] * b[0]) - f32(a[0] * b[2]), f32(a[0] * b[1]) - f32(a[1] * b[0])], f32)
        nrm, which = normalized(cr)
        cnt[which] += 1
        centre = (((p[0] + p[1]) + p[2]).astype(f64) / 3.0).astype(f32) * mult
        out_p.append(centre[None, :])
        big, iterA, iterB, pA, pB, branch = tri_plan(p)
        cnt[branch] += 1
        n = 1
        if big and (iterA == 0 or iterB == 0):
            cnt["iter_zero"] += 1
        if big and iterA > 0 and iterB > 0:
            u = (np.arange(iterA, dtype=f64) / f64(iterA)).astype(f32)[:, None]
            v = (np.arange(iterB, dtype=f64) / f64(iterB)).astype(f32)[None, :]
            w = (f32(1) - u) - v
            keep = ~(w < 0)
            cnt["skipped_w"] += int((~keep).sum())
            A, B, C = p[pA] * mult, p[pB] * mult, p[3 - pA - pB] * mult
            U, V = np.broadcast_to(u, w.shape)[keep], np.broadcast_to(v, w.shape)[keep]
            W = w[keep]
            q = (A[None, :] * U[:, None] + B[None, :] * V[:, None]) + C[None, :] * W[:, None]
            out_p.append(q.astype(f32))
            n += q.shape[0]
        out_n.append(np.broadcast_to(nrm, (n, 3)))
        per_tri.append(n)
    if not out_p:
        return np.zeros((0, 3), f32), np.zeros((0, 3), f32), cnt, np.zeros(0, np.int64)
    return np.concatenate(out_p).astype(f32), np.concatenate(out_n).astype(f32), cnt, np.array(per_tri, np.int64)


# ---- stage 2: binning ----------------------------------------------------------------------------------------------------------------
def cell_index(spos, dims):
    """_cIndex, mesh.cpp:822-826: truncation toward zero, then the bounds test; -1 outside"""
    sx, sy, sz = dims
    ok = np.isfinite(spos).all(1) & (np.abs(spos) < 2e9).all(1) if spos.size else np.zeros(0, bool)
    c = np.trunc(np.where(ok[:, None], spos, -5)).astype(np.int64)
    ok = ok & (c >= 0).all(1) & (c[:, 0] < sx) & (c[:, 1] < sy) & (c[:, 2] < sz)
    return np.where(ok, c[:, 0] + sx * (c[:, 1] + sy * c[:, 2]), -1)


def binning(spos, snrm, dims):
    n = dims[0] * dims[1] * dims[2]
    cell = cell_index(spos, dims)
    inside = np.nonzero(cell >= 0)[0]
    order = inside[np.argsort(cell[inside], kind="stable")]
    ln = np.bincount(cell[inside], minlength=n).astype(np.int32)
    start = (np.cumsum(ln) - ln).astype(np.int32)
    return {"len": ln, "start": start, "bpos": spos[order], "bnrm": snrm[order], "dropped": int((cell < 0).sum()), "binned": int(inside.size)}


# ---- stage 3: gather -----------------------------------------------------------------------------------------------------------------
def expw(a):
    """the weight: the fp64 exp of the fp32 argument, rounded once"""
    return np.exp(a.astype(f64)).astype(f32)


def gather(dims, B, P, weight=expw):
    """SDFKernel over every cell -> phi (pre-flood, unwritten cells -cutoff) and the fp64 counters n, S = sum w, A = sum |n.r| w.  The
    order of a cell's terms is i outer, j, k inner over the block, binned order within a cell: the same offset sequence for every cell,
    so the loop runs over offsets with all cells in flight."""
    sx, sy, sz = dims
    n = sx * sy * sz
    R = P["intRadius"]
    sum_, dist = np.zeros(n, f32), np.zeros(n, f32)
    cn, cS, cA = np.zeros(n, np.int64), np.zeros(n, f64), np.zeros(n, f64)
    occ = np.nonzero(B["len"])[0]
    oi, oj, ok = occ % sx, (occ // sx) % sy, occ // (sx * sy)
    olen, ostart = B["len"][occ], B["start"][occ]
    bp, bn = B["bpos"], B["bnrm"]
    # a cell at (source cell - offset) sees the source cell at +offset; offsets ascend with the source cell's i, j, k
    for di in range(-R, R + 1):
        for dj in range(-R, R + 1):
            for dk in range(-R, R + 1):
                if f32(f32(f32(di * di) + f32(dj * dj)) + f32(dk * dk)) > P["safeRadius2"]:
                    continue
                ci, cj, ck = oi - di, oj - dj, ok - dk
                m = (ci >= 0) & (cj >= 0) & (ck >= 0) & (ci < sx) & (cj < sy) & (ck < sz)
                if not m.any():
                    continue
                cell = (ci + sx * (cj + sy * ck))[m]
                cpos = np.stack([ci[m], cj[m], ck[m]], 1).astype(f32) + f32(0.5)
                ml, ms = olen[m], ostart[m]
                for q in range(int(ml.max())):
                    a = ml > q
                    s = ms[a] + q
                    c = cell[a]
                    r = cpos[a] - bp[s]
                    r2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
                    near = r2 < P["cutoff2"]
                    w = weight(-r2 * P["isigma2"])
                    dot = (bn[s, 0] * r[:, 0] + bn[s, 1] * r[:, 1]) + bn[s, 2] * r[:, 2]
                    c, w, dot = c[near], w[near], dot[near]
                    sum_[c] = sum_[c] + w                    # a cell occurs once per (offset, q): no repeated index
                    dist[c] = dist[c] + dot * w
                    cn[c] += 1
                    cS[c] += w.astype(f64)
                    cA[c] += np.abs(dot.astype(f64)) * w.astype(f64)
    written = sum_ > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = np.where(written, dist / np.where(written, sum_, f32(1)), -P["cutoff"]).astype(f32)
    return phi, {"n": cn, "S": cS, "A": cA, "written": written}


def bound(C, phi_ref):
    """|phi - phi_ref| <= (2 * 2^-23 + 4 n 2^-24) A / S + 2^-23 |phi_ref| per written cell"""
    S = np.where(C["S"] > 0, C["S"], 1.0)
    return (2 * 2.0 ** -23 + 4 * C["n"] * 2.0 ** -24) * C["A"] / S + 2.0 ** -23 * np.abs(phi_ref.astype(f64))


# ---- stage 4: flood fill -------------------------------------------------------------------------------------------------------------
def flood_closure(phi, dims, cutoff):
    """every seed (phi >= cutoff - 1) and every cell reachable from a seed through 6-neighbours whose value is < 0 holds cutoff.
    -> field, number of dilation steps"""
    sx, sy, sz = dims
    cutoff = f32(cutoff)
    v = phi.reshape(sz, sy, sx)
    inset = v >= f32(cutoff - f32(1.0))
    cand = v < 0
    steps = 0
    while True:
        nb = np.zeros_like(inset)
        nb[1:] |= inset[:-1]; nb[:-1] |= inset[1:]
        nb[:, 1:] |= inset[:, :-1]; nb[:, :-1] |= inset[:, 1:]
        nb[:, :, 1:] |= inset[:, :, :-1]; nb[:, :, :-1] |= inset[:, :, 1:]
        new = nb & cand & ~inset
        if not new.any():
            break
        inset |= new
        steps += 1
    return np.where(inset, cutoff, v).astype(f32).reshape(-1), steps


def flood_stack(phi, dims, cutoff):
    """the literal loop of mesh.cpp:989-1004"""
    sx, sy, sz = dims
    cutoff = f32(cutoff)
    v = phi.reshape(sz, sy, sx).copy()
    stack = [(i, j, k) for k in range(sz) for j in range(sy) for i in range(sx) if v[k, j, i] >= f32(cutoff - f32(1.0))]
    while stack:
        i, j, k = stack.pop()
        v[k, j, i] = cutoff
        if i > 0 and v[k, j, i - 1] < 0: stack.append((i - 1, j, k))
        if j > 0 and v[k, j - 1, i] < 0: stack.append((i, j - 1, k))
        if k > 0 and v[k - 1, j, i] < 0: stack.append((i, j, k - 1))
        if i < sx - 1 and v[k, j, i + 1] < 0: stack.append((i + 1, j, k))
        if j < sy - 1 and v[k, j + 1, i] < 0: stack.append((i, j + 1, k))
        if k < sz - 1 and v[k + 1, j, i] < 0: stack.append((i, j, k + 1))
    return v.reshape(-1)


def tile_rounds(phi, dims, cutoff, tile=8):
    """the rounds of the device's statement: per round every tile runs to its fixed point with the halo as the round began.  -> field,
    rounds launched (the last one changes nothing).  A device round may see a neighbour's change early, so its count is at most this."""
    sx, sy, sz = dims
    cutoff = f32(cutoff)
    v = phi.reshape(sz, sy, sx).copy()
    v[v >= f32(cutoff - f32(1.0))] = cutoff
    rounds = 0
    while True:
        rounds += 1
        old = v.copy()
        for k0 in range(0, sz, tile):
            for j0 in range(0, sy, tile):
                for i0 in range(0, sx, tile):
                    lo = (max(k0 - 1, 0), max(j0 - 1, 0), max(i0 - 1, 0))
                    hi = (min(k0 + tile + 1, sz), min(j0 + tile + 1, sy), min(i0 + tile + 1, sx))
                    sub = old[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
                    inner = np.zeros(sub.shape, bool)
                    inner[k0 - lo[0]:k0 - lo[0] + tile, j0 - lo[1]:j0 - lo[1] + tile, i0 - lo[2]:i0 - lo[2] + tile] = True
                    inset, cand = sub == cutoff, (sub < 0) & inner
                    if not cand.any():
                        continue
                    while True:
                        nb = np.zeros_like(inset)
                        nb[1:] |= inset[:-1]; nb[:-1] |= inset[1:]
                        nb[:, 1:] |= inset[:, :-1]; nb[:, :-1] |= inset[:, 1:]
                        nb[:, :, 1:] |= inset[:, :, :-1]; nb[:, :, :-1] |= inset[:, :, 1:]
                        new = nb & cand & ~inset
                        if not new.any():
                            break
                        inset |= new
                    blk = v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
                    blk[inset & inner] = cutoff
        if np.array_equal(v.view(np.uint32), old.view(np.uint32)):
            return v.reshape(-1), rounds


# ---- the whole thing -----------------------------------------------------------------------------------------------------------------
def mesh_sdf(pos, tris, mesh_gs, dims, sigma, cutoff=-1., weight=expw):
    P = params(sigma, cutoff)
    mult = np.array(dims, f32) / np.array(mesh_gs, f32)
    spos, snrm, cnt, per_tri = sources(pos, tris, mult)
    B = binning(spos, snrm, dims)
    pre, C = gather(dims, B, P, weight)
    phi, steps = flood_closure(pre, dims, P["cutoff"])
    cnt.update(dropped=B["dropped"], binned=B["binned"], sources=spos.shape[0], flood_steps=steps,
               flooded=int((phi.view(np.uint32) != pre.view(np.uint32)).sum()), written=int(C["written"].sum()),
               max_in_cell=int(B["len"].max()) if B["len"].size else 0, max_n=int(C["n"].max()))
    return {"P": P, "spos": spos, "snrm": snrm, "per_tri": per_tri, "bin": B, "pre": pre, "C": C, "phi": phi, "counters": cnt}


def margin_ok(R):
    """the conditions that go with the tolerance: no pre-flood value of a written cell within its bound of cutoff - 1 or of 0"""
    pre, C, c = R["pre"].astype(f64), R["C"], f64(R["P"]["cutoff"])
    b = bound(C, R["pre"])
    w = C["written"] & (C["A"] > 0)          # every n.r zero (zero-area triangles): phi is a zero whatever the weights are
    return bool((np.abs(pre[w] - (c - 1.0)) > b[w]).all() and (np.abs(pre[w]) > b[w]).all())


def apply_mesh_to_grid(grid, sdf, value, flags=None):
    """ApplyMeshToGrid, mesh.cpp:829-837; grid [n] or [3][n]"""
    m = sdf < 0
    if flags is not None:
        m &= (flags & 2) == 0
    out = grid.copy()
    if out.ndim == 1:
        out[m] = value
    else:
        for c in range(3):
            out[c][m] = value[c]
    return out


def apply_density(flags, density, sdf, value, sigma):
    """KnApplyDensity, initplugins.cpp:132-137"""
    out = density.copy()
    out[((flags & 1) != 0) & ~(sdf > f32(sigma))] = f32(value)
    return out


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def uv_sphere(centre, radius, nu=10, nv=6):
    """a closed lat-long sphere, outward normals"""
    pos = [(0, 0, 1)]
    for a in range(1, nv):
        th = np.pi * a / nv
        for b in range(nu):
            ph = 2 * np.pi * b / nu
            pos.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    pos.append((0, 0, -1))
    tris = []
    ring = lambda a, b: 1 + (a - 1) * nu + b % nu
    for b in range(nu):
        tris.append((0, ring(1, b), ring(1, b + 1)))
        tris.append((len(pos) - 1, ring(nv - 1, b + 1), ring(nv - 1, b)))
    for a in range(1, nv - 1):
        for b in range(nu):
            tris.append((ring(a, b), ring(a + 1, b), ring(a + 1, b + 1)))
            tris.append((ring(a, b), ring(a + 1, b + 1), ring(a, b + 1)))
    return (np.array(pos, f64) * radius + np.array(centre, f64)).astype(f32), np.array(tris, np.int32)


def tri_from_lengths(l0, l1, l2, origin, seed):
    """a triangle with |edge 0| = l0 (node 1 - node 0), |edge 1| = l1, |edge 2| = l2 in a tilted plane"""
    rng = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rng.randn(3, 3))
    x = (l0 * l0 + l2 * l2 - l1 * l1) / (2 * l0)
    y = np.sqrt(max(l2 * l2 - x * x, 0.0))
    p = np.array([(0, 0, 0), (l0, 0, 0), (x, y, 0)], f64) @ q.T + np.array(origin, f64)
    return p.astype(f32), np.array([(0, 1, 2)], np.int32)


def random_tris(n, dims, seed, size=0.6):
    rng = np.random.RandomState(seed)
    c = rng.rand(n, 1, 3) * (np.array(dims, f64) + 1.0) - 0.5          # some centres fall outside the grid
    p = (c + (rng.rand(n, 3, 3) - 0.5) * size).reshape(-1, 3).astype(f32)
    return p, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def load_obj(path):
    """the v / f records of an .obj (1-based, `a/b/c` corners): what Mesh.load keeps, before any transform"""
    pos, tris = [], []
    for line in open(path):
        t = line.split()
        if not t:
            continue
        if t[0] == "v":
            pos.append([float(x) for x in t[1:4]])
        elif t[0] == "f":
            tris.append([int(x.split("/")[0]) - 1 for x in t[1:4]])
    return np.array(pos, f32), np.array(tris, np.int32)


SC_SHIFT = (0.17, -0.21, 0.07)
BIG_PATTERNS = {  # bigEdges -> (l0, l1, l2) with exactly those edges above 0.75; "s": every count 0 or 1, "l": samples where the shape allows
    "big1s": (0.9, 0.6, 0.6), "big2s": (0.6, 0.9, 0.6), "big4s": (0.6, 0.6, 0.9), "big3s": (0.9, 0.9, 0.5), "big5s": (0.9, 0.5, 0.9),
    "big6s": (0.5, 0.9, 0.9), "big7s": (1.0, 1.1, 1.2), "big1l": (1.45, 0.74, 0.74), "big2l": (0.74, 1.45, 0.74), "big4l": (0.74, 0.74, 1.45),
    "big3l": (5.0, 5.2, 0.5), "big5l": (5.0, 0.5, 5.2), "big6l": (0.5, 5.0, 5.2), "big7l": (4.0, 5.0, 6.0),
}
BIG_EXPECT = {"big1": 1, "big2": 2, "big4": 4, "big3": 3, "big5": 5, "big6": 6, "big7": 7}


def _case(dims, pos, tris, sigma=2., cutoff=-1., mesh_gs=None):
    return {"dims": tuple(dims), "mesh_gs": tuple(mesh_gs or dims), "pos": np.asarray(pos, f32).reshape(-1, 3),
            "tris": np.asarray(tris, np.int32).reshape(-1, 3), "sigma": float(sigma), "cutoff": float(cutoff)}


def _cat(parts):
    pos, tris, base = [], [], 0
    for p, t in parts:
        pos.append(p)
        tris.append(t + base)
        base += p.shape[0]
    return np.concatenate(pos), np.concatenate(tris)


@functools.lru_cache(maxsize=None)
def case(name):
    D = (12, 11, 10)
    if name == "empty":
        return _case(D, np.zeros((0, 3)), np.zeros((0, 3)))
    if name == "one":
        return _case(D, [(5.1, 5.2, 5.3), (5.6, 5.2, 5.4), (5.3, 5.7, 5.2)], [(0, 1, 2)])
    if name == "outside":
        return _case(D, [(15.1, 5.2, 5.3), (15.6, 5.2, 5.4), (15.3, 5.7, 5.2)], [(0, 1, 2)])
    if name == "faces":
        # centres exactly at -0.5 / on the upper faces / just inside them: offsets that sum to zero exactly
        off = np.array([(0.25, 0.0625, 0.125), (0, 0.25, -0.25), (-0.25, -0.3125, 0.125)], f64)
        cs = [(-0.5, 3.5, 3.5), (3.5, -0.5, 3.5), (3.5, 3.5, -0.5), (-0.5, -0.5, -0.5), (12.0, 5.5, 5.5), (5.5, 11.0, 5.5), (5.5, 5.5, 10.0),
              (11.75, 10.75, 9.75), (-1.0, 5.5, 5.5), (5.5, 5.5, -1.25)]
        return _case(D, np.concatenate([np.array(c) + np.roll(off, q, 1) * (0.5 if q % 2 else 1) for q, c in enumerate(cs)]),
                     np.arange(3 * len(cs)).reshape(-1, 3))
    if name == "zero_area":
        return _case(D, [(5.5, 5.5, 5.5), (6.5, 5.5, 5.5), (7.5, 5.5, 5.5), (4.25, 4.5, 4.5), (4.25, 4.5, 4.5), (4.25, 4.5, 4.5),
                         (6.1, 6.2, 6.3), (6.6, 6.2, 6.4), (6.3, 6.7, 6.2)], [(0, 1, 2), (3, 4, 5), (6, 7, 8)])
    if name in BIG_PATTERNS:
        p, t = tri_from_lengths(*BIG_PATTERNS[name], origin=(5.0, 5.0, 4.5), seed=len(name) + sum(map(ord, name)))
        return _case(D, p, t)
    if name == "span":
        # two triangles across a 33x31x29 grid given in a mesh solver three times as fine: thousands of samples each
        p = np.array([(4, 5, 6), (95, 8, 40), (50, 88, 80), (90, 85, 10)], f64)
        return _case((33, 31, 29), p, [(0, 1, 2), (1, 3, 2)], mesh_gs=(99, 93, 87))
    if name == "dense":
        rng = np.random.RandomState(11)
        c = np.array((6.5, 5.5, 4.5)) + (rng.rand(210, 1, 3) - 0.5) * 0.5
        p = c + (rng.rand(210, 3, 3) - 0.5) * 0.3
        return _case(D, p.reshape(-1, 3), np.arange(630).reshape(-1, 3))
    if name.startswith("rand"):
        n = int(name[4:])
        dims = (33, 31, 29) if n >= 1000 else D
        return _case(dims, *random_tris(n, dims, 100 + n))
    if name.startswith("sc_"):          # sc_<sigma>_<cutoff>_<dims>: a sphere that fits the grid
        _, sg, co, dm = name.split("_")
        dims = {"754": (7, 5, 4), "666": (6, 6, 6), "big": (33, 31, 29)}[dm]
        r = 0.3 * min(dims)
        ctr = np.array(dims) * 0.5 + np.array(SC_SHIFT)
        return _case(dims, *uv_sphere(ctr, r, 8 if dm != "big" else 14, 5 if dm != "big" else 9), sigma=float(sg), cutoff=float(co))
    if name == "row65":
        return _case((65, 3, 3), *_cat([random_tris(40, (65, 3, 3), 5), uv_sphere((20.3, 1.4, 1.6), 1.2, 6, 4)]))
    if name == "col70":
        return _case((3, 3, 70), *_cat([random_tris(40, (3, 3, 70), 6), uv_sphere((1.4, 1.6, 50.3), 1.2, 6, 4)]))
    if name == "mult":
        return _case((18, 15, 21), *uv_sphere((6.2, 5.9, 6.1), 3.6, 10, 7), mesh_gs=(12, 12, 12))
    if name == "sphere_closed":
        return _case((28, 28, 28), *uv_sphere((14.2, 13.9, 14.1), 10.0, 6, 4), sigma=1., cutoff=2.)
    if name == "sphere_open":
        p, t = uv_sphere((14.2, 13.9, 14.1), 10.0, 6, 4)
        return _case((28, 28, 28), p, np.delete(t, 14, 0), sigma=1., cutoff=2.)
    if name in OBJ_CASES:
        fname, res, shift = OBJ_CASES[name]
        p, t = load_obj(os.path.join(GOLD, fname))
        return _case((res, res, res), obj_placed(p, res, shift), t)
    raise KeyError(name)


def obj_offset(res, shift):
    """gs * (Vec3(0.5) + shift) in the reference's fp32 vector arithmetic"""
    return (np.array((0.5, 0.5, 0.5), f32) + np.array(shift, f32)) * f32(res)


def obj_placed(pos, res, shift):
    """mesh.scale(vec3(res / 3.0)) then mesh.offset(gs * (Vec3(0.5) + shift)) as the two scripts do it, in fp32"""
    return pos * f32(res / 3.0) + obj_offset(res, shift)


# the reference's two scripts at small sizes: tools/tests/test_0050_meshload.py (res 100 there) and scenes/meshload.py (res 50 there)
OBJ_CASES = {"obj0050": ("test_0050_meshload.obj", 32, (0, 0, 0)), "torus24": ("simpletorus.obj", 24, (0.1, 0.05, 0))}
SC_CASES = ["sc_%s_%s_%s" % (sg, co, dm) for dm in ("754", "666", "big") for sg in ("1", "2", "2.5") for co in ("-1", "3", "7")]
CASES = (["empty", "one", "outside", "faces", "zero_area"] + sorted(BIG_PATTERNS) + ["span", "dense"] +
         ["rand%d" % n for n in (1, 63, 64, 65, 5000)] + SC_CASES + ["row65", "col70", "mult", "sphere_closed", "sphere_open"] + sorted(OBJ_CASES))


@functools.lru_cache(maxsize=None)
def model(name):
    c = case(name)
    return mesh_sdf(c["pos"], c["tris"], c["mesh_gs"], c["dims"], c["sigma"], c["cutoff"])


def reference_phi(G, name):
    """the reference's field from the fixture: the model's with the recorded differing cells patched in, checked by its digest"""
    ref = model(name)["phi"].copy()
    idx = G[name + "/diff_idx"]
    ref[idx] = G[name + "/diff_val"]
    assert np.array_equal(sha(ref), G[name + "/sha"]), "%s: the patched model field does not have the reference's digest" % name
    if (name + "/phi") in G.files:
        assert np.array_equal(G[name + "/phi"].view(np.uint32), ref.view(np.uint32)), name
    return ref


# ---- synthetic fields for the flood fill alone -----------------------------------------------------------------------------------------
def flood_field(name):
    """-> dims, phi, cutoff"""
    if name == "snake":
        # a U-shaped channel of candidates in a field of 0.5 (neither seed nor candidate), the seed at one end: down one arm, across, up
        dims = (20, 20, 12)
        v = np.full(dims[::-1], 0.5, f32)
        v[5, 2:18, 3] = -1
        v[5, 17, 3:17] = -1
        v[5, 2:18, 16] = -1
        v[5, 2, 3] = 3.5
        return dims, v.reshape(-1), 4.0
    if name == "corner":
        dims = (24, 20, 17)
        v = np.full(dims[::-1], -4.0, f32)
        v[:3, :3, :3] = 3.5
        v[8:12, 5:15, 6:18] = 0.25          # a block that is neither
        v[9:11, 7:12, 8:14] = -1.0          # and an enclosed pocket that must stay
        return dims, v.reshape(-1), 4.0
    rng = np.random.RandomState(int(name[4:]))
    dims = tuple(int(x) for x in rng.randint(1, 12, 3))
    cutoff = float(rng.choice([0.0, 0.5, 1.0, 2.0, 4.0]))
    v = rng.choice(np.array([-4, -1, -0.25, 0, 0.25, cutoff - 1, cutoff, cutoff + 1, cutoff - 1.5], f32), size=dims[::-1],
                   p=[.25, .2, .1, .1, .15, .03, .03, .04, .1])
    return dims, v.reshape(-1).astype(f32), cutoff


# ---- densityInflowMesh (initplugins.cpp:147-152): computeLevelset(sdf, 2., cutoff) then KnApplyDensity --------------------------------
INFLOW_CASE = "sc_2_7_big"
INFLOW_ARGS = ((1.0, 7.0, 0.0), (0.75, 3.0, 0.5))        # value, cutoff, sigma


def inflow_inputs(name):
    """-> flags (fluid / obstacle / empty at random), density"""
    rng = np.random.RandomState(77)
    n = int(np.prod(case(name)["dims"]))
    return rng.choice(np.array([1, 2, 4], np.int32), n, p=[.7, .15, .15]), rng.rand(n).astype(f32)


@functools.lru_cache(maxsize=None)
def inflow_sdf(name, cutoff):
    c = case(name)
    return mesh_sdf(c["pos"], c["tris"], c["mesh_gs"], c["dims"], 2., cutoff)["phi"]


def inflow_model(name, q):
    value, cutoff, sigma = INFLOW_ARGS[q]
    flags, dens = inflow_inputs(name)
    return apply_density(flags, dens, inflow_sdf(name, cutoff), value, sigma)


# ---- the loop of scenes/meshload.py, recorded from the reference at a small size --------------------------------------------------------
LOOP_CASE, LOOP_STEPS = "torus24", 6


def loop_cylinder(res):
    """centre, radius, z of the script's source = Cylinder(center=gs*vec3(0.35,0.2,0.5), radius=res*0.15, z=gs*vec3(0, 0.05, 0)) as the
    script's Python floats, rounded to fp32"""
    return np.array([res * 0.35, res * 0.2, res * 0.5, res * 0.15, res * 0.0, res * 0.05, res * 0.0], f32)
