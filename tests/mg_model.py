"""A plain numpy statement of the reference's GridMg (source/multigrid.cpp) in its types and summation orders: the set-up of
setA (vertex activation, the greedy coarse-vertex selection with the bucket heap, the Galerkin operators) and the passes of one
V-cycle (the two- and eight-colour Gauss-Seidel smoother in both directions, the residual, restriction with x = 0,
interpolate-and-add, the coarsest-level CG in fp64).  tests/test_mg_model.py ties it to the two recorded fixtures
(tests/golden/multigrid_levels.npz of tools/record_mg_levels.py, and the stage__ entries of tests/golden/multigrid.npz),
tests/test_gpu_mg_levels.py compares the HIP library with it level by level.

Every pass is vectorised over the vertices of one colour or one pass: their results do not depend on each other, and the
per-vertex order of the terms (z, y, x from -1, as FOR_VEC_MINMAX loops) is kept.  fp32 products and sums are formed one
operation at a time (the reference is compiled without contraction); the CG's three sums run in vertex order (np.cumsum).

THE LEVEL-1 OPERATOR.  The reference sums level 1 over a list of precomputed paths that it sorts with std::sort under a
comparator that leaves ties, so the order of the terms inside one stencil entry belongs to the sorting algorithm and a model
cannot own it.  operator1() therefore forms the sums in the generic loop order of the levels > 1, once in fp32 and once in
fp64, and hands out its result only where the two agree exactly.  They agree for every integer system (MakeLaplaceMatrix
without fractions): the terms are small integers times multiples of 1/64, every partial sum is exact, so every order gives the
same bits -- setup() raises if they do not agree and it was given nothing else.  For other systems (ghost-fluid diagonals,
fill fractions) agreement of the two sums does not make the bits order-free (another order may round on the way), and the
caller must pass in the recorded level-1 operator (A1, or A1_patch as the fixture stores it); the model then owns the types and
everything from level 2 on, given that operator.

Layout: vertex v = x + sx * (y + sy * z); arrays per level are flat, operators are (4, n) on level 0 (A0, Ai, Aj, Ak) and
(14, n) above (plane s = stencil entry 13 + s of the 27-point stencil).  Types: 0 inactive, 1 active, 2 active trivial."""
import numpy as np

f32, f64 = np.float32, np.float64
INACTIVE, ACTIVE, TRIVIAL = 0, 1, 2
TRIVIAL_SCALE = f32(1e-6)


# ---------------------------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------------------------
def level_sizes(dims):
    """GridMg::GridMg: coarsen by (s + 2) / 2 until every dimension is <= 5 or the level has <= 1000 vertices"""
    sizes = [tuple(int(d) for d in dims)]
    while True:
        sx, sy, sz = sizes[-1]
        if (sx <= 5 and sy <= 5 and sz <= 5) or sx * sy * sz <= 1000 or len(sizes) > 100:
            return sizes
        sizes.append(((sx + 2) // 2, (sy + 2) // 2, (sz + 2) // 2))


def _coords(size):
    sx, sy, sz = size
    v = np.arange(sx * sy * sz)
    return v % sx, (v // sx) % sy, v // (sx * sy)


def _lin(size, X, Y, Z):
    return X + size[0] * (Y + size[1] * Z)


def _inside(size, X, Y, Z):
    return (X >= 0) & (Y >= 0) & (Z >= 0) & (X < size[0]) & (Y < size[1]) & (Z < size[2])


def _gather(a, idx, ok):
    """a[idx] where ok (idx may be anything elsewhere)"""
    return a[np.where(ok, idx, 0)]


# ---------------------------------------------------------------------------------------------------------
# set-up
# ---------------------------------------------------------------------------------------------------------
def activate(size, A0, Ai, Aj, Ak):
    """knCopyA + knActivateVertices + analyzeStencil -> types, level-0 operator (4, n), nonZeroStencilSumFound, trivialEquationsFound"""
    n = size[0] * size[1] * size[2]
    a = [np.asarray(p, f32).reshape(n) for p in (A0, Ai, Aj, Ak)]
    X, Y, Z = _coords(size)
    v = np.arange(n)
    py, pz = size[0], size[0] * size[1]
    lo = [np.where(X != 0, _gather(a[1], v - 1, X != 0), f32(0)), np.where(Y != 0, _gather(a[2], v - py, Y != 0), f32(0)),
          np.where(Z != 0, _gather(a[3], v - pz, Z != 0), f32(0))]
    st = a + lo
    ssum, smax = np.zeros(n, f32), np.zeros(n, f32)
    for s in st:
        ssum = ssum + s
        smax = np.maximum(smax, np.abs(s))
    act = a[0] != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        nonzero = bool((act & (np.abs(ssum / smax) > f32(1e-6))).any())
    triv = act & (a[0] == 1)
    for s in st[1:]:
        triv &= s == 0
    t = np.where(triv, TRIVIAL, np.where(act, ACTIVE, INACTIVE)).astype(np.uint8)
    A = np.stack(a).copy()
    A[0] = np.where(triv, A[0] * TRIVIAL_SCALE, A[0])
    return t, A, nonzero, bool(triv.any())


class BucketHeap(object):
    """NKMinHeap: one doubly linked list per key; set_key puts an ID at the HEAD of its key's list, pop_min takes the head of
    the smallest non-empty key"""

    def __init__(self, n, k):
        self.K, self.size = k, 0
        self.key, self.prev, self.next = [-1] * (n + k), [-1] * (n + k), [-1] * (n + k)

    def get_key(self, i):
        return self.key[self.K + i]

    def _unlink(self, e):
        pr, su = self.prev[e], self.next[e]
        self.next[pr] = su
        if su != -1:
            self.prev[su] = pr

    def set_key(self, i, k):
        e = self.K + i
        if self.key[e] == k:
            return
        if self.key[e] != -1:
            self._unlink(e)
            self.size -= 1
        self.key[e] = k
        if k == -1:
            self.next[e] = self.prev[e] = -1
            return
        self.size += 1
        old = self.next[k]
        self.next[k], self.prev[e], self.next[e] = e, k, old
        if old != -1:
            self.prev[old] = e

    def pop_min(self):
        k = 0
        while self.next[k] == -1:
            k += 1
        e = self.next[k]
        self._unlink(e)
        self.key[e] = self.prev[e] = self.next[e] = -1
        self.size -= 1
        return e - self.K


def select_coarse(fsize, tf, csize, heap_cls=BucketHeap):
    """genCoarseGrid + knActivateCoarseVertices: the types of the coarse level from those of the fine one"""
    FREE, ZERO, REMOVED = 5, 4, 3
    fx, fy, fz = fsize
    cx, cy, cz = csize
    tc = [FREE] * (cx * cy * cz)
    heap = heap_cls(fx * fy * fz, 9)
    tf = np.asarray(tf)
    X, Y, Z = _coords(fsize)
    fiv = 1 << ((X & 1) + (Y & 1) + (Z & 1))
    for v in np.nonzero(tf != INACTIVE)[0].tolist():
        heap.set_key(v, int(fiv[v]))
    while heap.size > 0:
        v = heap.pop_min()
        x, y, z = v % fx, (v // fx) % fy, v // (fx * fy)
        vdone = False
        for iz in range(z // 2, (z + 1) // 2 + 1):
            for iy in range(y // 2, (y + 1) // 2 + 1):
                for ix in range(x // 2, (x + 1) // 2 + 1):
                    i = ix + cx * (iy + cy * iz)
                    if tc[i] != FREE:
                        continue
                    if vdone:
                        tc[i] = REMOVED
                    else:
                        tc[i] = ZERO
                        vdone = True
                    for rz in range(max(0, iz * 2 - 1), min(fz - 1, iz * 2 + 1) + 1):
                        for ry in range(max(0, iy * 2 - 1), min(fy - 1, iy * 2 + 1) + 1):
                            for rx in range(max(0, ix * 2 - 1), min(fx - 1, ix * 2 + 1) + 1):
                                r = rx + fx * (ry + fy * rz)
                                k = heap.get_key(r)
                                if k > 1:
                                    heap.set_key(r, k - 1)
                                elif k > -1:
                                    heap.set_key(r, -1)
    return np.array([ACTIVE if c == ZERO else INACTIVE for c in tc], np.uint8)


def _pow2inv(X, Y, Z, dtype):
    return (1.0 / (1 << ((X & 1) + (Y & 1) + (Z & 1)))).astype(dtype)


_OFF = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]      # s = 0..26


def _galerkin(fsize, tf, Af, csize, tc, dtype, seven):
    """knGenCoarseGridOperator in the loop order of the levels > 1: U (restriction vertices of V), N (coarse neighbours reached
    through U, entries sc >= 13 only), W (the stencil of U that interpolates from N); truncating divisions as in C.
    seven: the fine level stores the 7-point stencil in 4 planes (level 0), else the 27-point stencil in 14 planes."""
    nc = csize[0] * csize[1] * csize[2]
    VX, VY, VZ = _coords(csize)
    actf, actc = np.asarray(tf) != INACTIVE, np.asarray(tc) != INACTIVE
    Af = np.asarray(Af).astype(dtype)
    A = np.zeros((14, nc), dtype)
    seven_sf = {13: (0, True), 14: (1, True), 12: (1, False), 16: (2, True), 10: (2, False), 22: (3, True), 4: (3, False)}
    for d in _OFF:
        UX, UY, UZ = VX * 2 + d[0], VY * 2 + d[1], VZ * 2 + d[2]
        oku = _inside(fsize, UX, UY, UZ)
        u = _lin(fsize, UX, UY, UZ)
        oku = oku & _gather(actf, u, oku) & actc
        if not oku.any():
            continue
        rw = _pow2inv(UX, UY, UZ, dtype)
        for m in _OFF:
            sc = (m[0] + 1) + 3 * (m[1] + 1) + 9 * (m[2] + 1)
            if sc < 13:
                continue
            NX, NY, NZ = VX + m[0], VY + m[1], VZ + m[2]
            okn = oku & _inside(csize, NX, NY, NZ)
            for Uc, Nc in ((UX, NX), (UY, NY), (UZ, NZ)):
                # (U - 1) / 2 <= N <= (U + 2) / 2, the lower bound truncating towards zero (U = 0 gives 0; N >= 0 holds already)
                okn = okn & (Nc >= np.floor_divide(Uc - 1, 2)) & (Nc <= np.floor_divide(Uc + 2, 2))
            nn = _lin(csize, NX, NY, NZ)
            okn = okn & _gather(actc, nn, okn)
            if not okn.any():
                continue
            acc = A[sc - 13]
            for sf, e in enumerate(_OFF):
                if seven and sf not in seven_sf:
                    continue
                if any(abs(d[c] + e[c] - 2 * m[c]) > 1 for c in range(3)):      # W within N * 2 -+ 1 on every axis
                    continue
                WX, WY, WZ = UX + e[0], UY + e[1], UZ + e[2]
                okw = okn & _inside(fsize, WX, WY, WZ)
                w = _lin(fsize, WX, WY, WZ)
                okw = okw & _gather(actf, w, okw)
                if not okw.any():
                    continue
                if seven:
                    plane, in_u = seven_sf[sf]
                else:
                    plane, in_u = (13 - sf, False) if sf < 14 else (sf - 13, True)
                a = _gather(Af[plane], u if in_u else w, okw)
                iw = _pow2inv(WX, WY, WZ, dtype)
                acc = np.where(okw, acc + rw * a * iw, acc)
            A[sc - 13] = acc
    return A


def operator1(size0, t0, A0, size1, t1):
    """the level-1 operator where its bits do not depend on the order of the reference's sorted paths -> (14, n1) fp32, and the
    mask of the entries that are owned (see the module's docstring)"""
    a32 = _galerkin(size0, t0, A0, size1, t1, f32, True)
    a64 = _galerkin(size0, t0, A0, size1, t1, f64, True)
    return a32, a32.astype(f64) == a64


def operatorN(fsize, tf, Af, csize, tc):
    return _galerkin(fsize, tf, Af, csize, tc, f32, False)


class Hierarchy(object):
    pass


def setup(dims, A, A1=None, A1_patch=None, types=None):
    """GridMg::setA.  A: the four planes of the system.  For a system whose level-1 sums are not exact, the recorded level-1
    operator: A1, the (14, n1) array, or A1_patch, the same as (flat indices, values) of the entries in which it differs from
    operator1()'s fp32 sums (how tests/golden/multigrid_levels.npz stores it).  types: the types of the levels > 0, to skip the
    (serial, slow) selection where a caller has them from a fixture that was checked elsewhere."""
    H = Hierarchy()
    H.sizes = level_sizes(dims)
    H.nl = len(H.sizes)
    t0, A0, H.nonzero_sum_found, H.trivial_found = activate(H.sizes[0], *A)
    H.t, H.A = [t0], [A0]
    for l in range(1, H.nl):
        t = np.asarray(types[l], np.uint8) if types is not None else select_coarse(H.sizes[l - 1], H.t[l - 1], H.sizes[l])
        if l == 1:
            op, own = operator1(H.sizes[0], t0, A0, H.sizes[1], t)
            H.A1_owned = own
            if A1 is not None:
                op = np.array(A1, f32).reshape(op.shape)
            elif A1_patch is not None:
                op = op.copy()
                op.reshape(-1)[np.asarray(A1_patch[0], np.int64)] = np.asarray(A1_patch[1], f32)
            elif not own.all():
                raise ValueError("level-1 operator: %d entries depend on the order of the reference's sorted paths; pass the recorded operator" % (~own).sum())
        else:
            op = operatorN(H.sizes[l - 1], H.t[l - 1], H.A[l - 1], H.sizes[l], t)
        H.t.append(t)
        H.A.append(op)
    H.active = [int((t != INACTIVE).sum()) for t in H.t]
    return H


# ---------------------------------------------------------------------------------------------------------
# the passes
# ---------------------------------------------------------------------------------------------------------
def _row0(size, A, x, start, diag=False):
    """start - the 7-point row of level 0 at every vertex: per axis the lower neighbour, then the upper one (knSmoothColor,
    knCalcResidual); diag subtracts the centre last"""
    X, Y, Z = _coords(size)
    v = np.arange(x.size)
    s = start
    for plane, c, dim, pitch in ((1, X, size[0], 1), (2, Y, size[1], size[0]), (3, Z, size[2], size[0] * size[1])):
        ok = c > 0
        s = np.where(ok, s - _gather(A[plane], v - pitch, ok) * _gather(x, v - pitch, ok), s)
        ok = c < dim - 1
        s = np.where(ok, s - A[plane] * _gather(x, v + pitch, ok), s)
    if diag:
        s = s - A[0] * x
    return s


def _row27(size, t, A, x, start, skip_centre=False):
    """start - the 27-point row of a level > 0 in the s order (knSmoothColor without the centre, knCalcResidual with it)"""
    X, Y, Z = _coords(size)
    act = t != INACTIVE
    s = start
    for si, (dx, dy, dz) in enumerate(_OFF):
        if skip_centre and si == 13:
            continue
        NX, NY, NZ = X + dx, Y + dy, Z + dz
        ok = _inside(size, NX, NY, NZ)
        nn = _lin(size, NX, NY, NZ)
        ok = ok & _gather(act, nn, ok)
        a = _gather(A[13 - si], nn, ok) if si < 14 else A[si - 13]
        s = np.where(ok, s - a * _gather(x, nn, ok), s)
    return s


def smooth(H, l, x, b, reverse):
    """smoothGS: two colours on level 0 (the parity of x + y + z), eight above (the offset in the 2 x 2 x 2 blocks)"""
    size, t, A = H.sizes[l], H.t[l], H.A[l]
    X, Y, Z = _coords(size)
    act = t != INACTIVE
    colours = list(range(2 if l == 0 else 8))
    for c in (reversed(colours) if reverse else colours):
        if l == 0:
            mine = ((X + Y + Z) & 1) == c
            s = _row0(size, A, x, b)
        else:
            mine = ((X & 1) == (c & 1)) & ((Y & 1) == ((c >> 1) & 1)) & ((Z & 1) == (c >> 2))
            s = _row27(size, t, A, x, b, skip_centre=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.where(mine & act, s / A[0], x)
    return x


def residual(H, l, x, b, r):
    size, t, A = H.sizes[l], H.t[l], H.A[l]
    s = _row0(size, A, x, b, diag=True) if l == 0 else _row27(size, t, A, x, b)
    return np.where(t != INACTIVE, s, r)


def restrict(H, lc, r_fine, b_coarse):
    """knRestrict: b of level lc from r of level lc - 1 (inactive coarse vertices keep their b)"""
    fsize, csize = H.sizes[lc - 1], H.sizes[lc]
    VX, VY, VZ = _coords(csize)
    actf = H.t[lc - 1] != INACTIVE
    s = np.zeros(VX.size, f32)
    for dx, dy, dz in _OFF:
        RX, RY, RZ = VX * 2 + dx, VY * 2 + dy, VZ * 2 + dz
        ok = _inside(fsize, RX, RY, RZ)
        r = _lin(fsize, RX, RY, RZ)
        ok = ok & _gather(actf, r, ok)
        s = np.where(ok, s + _pow2inv(RX, RY, RZ, f32) * _gather(r_fine, r, ok), s)
    return np.where(H.t[lc] != INACTIVE, s, b_coarse)


def interp_add(H, lf, x_coarse, x_fine):
    """knInterpolate into r + knAddAssign(x, r) on the active vertices of level lf"""
    fsize, csize = H.sizes[lf], H.sizes[lf + 1]
    X, Y, Z = _coords(fsize)
    actc = H.t[lf + 1] != INACTIVE
    s = np.zeros(X.size, f32)
    for jz in (0, 1):
        for jy in (0, 1):
            for jx in (0, 1):
                ok = ((jx == 0) | ((X & 1) == 1)) & ((jy == 0) | ((Y & 1) == 1)) & ((jz == 0) | ((Z & 1) == 1))
                i = _lin(csize, X // 2 + jx, Y // 2 + jy, Z // 2 + jz)
                ok = ok & _gather(actc, i, ok)
                s = np.where(ok, s + _gather(x_coarse, i, ok), s)
    c = _pow2inv(X, Y, Z, f32) * s
    return np.where(H.t[lf] != INACTIVE, x_fine + c, x_fine)


def _ordered_sum(a):
    """a[0] + a[1] + ... one after the other in fp64"""
    return f64(np.cumsum(a, dtype=f64)[-1]) if a.size else f64(0)


def _cg_terms(H, l):
    """the row of applyAStencil at the active vertices as (terms, active) arrays: neighbour index, coefficient (fp64), present?"""
    size, t, A = H.sizes[l], H.t[l], H.A[l]
    av = np.nonzero(t != INACTIVE)[0]
    X, Y, Z = (c[av] for c in _coords(size))
    idx, coef, ok = [], [], []
    if l == 0:
        for plane, c, dim, pitch in ((1, X, size[0], 1), (2, Y, size[1], size[0]), (3, Z, size[2], size[0] * size[1])):
            for o, n, src in ((c > 0, av - pitch, av - pitch), (c < dim - 1, av + pitch, av)):
                ok.append(o); idx.append(np.where(o, n, 0)); coef.append(A[plane][np.where(o, src, 0)])
        ok.append(np.ones(av.size, bool)); idx.append(av); coef.append(A[0][av])
    else:
        act = t != INACTIVE
        for si, (dx, dy, dz) in enumerate(_OFF):
            o = _inside(size, X + dx, Y + dy, Z + dz)
            n = np.where(o, _lin(size, X + dx, Y + dy, Z + dz), 0)
            o = o & act[n]
            ok.append(o); idx.append(np.where(o, n, 0)); coef.append(A[13 - si][n] if si < 14 else A[si - 13][av])
    return av, np.array(idx), np.array(coef).astype(f64), np.array(ok)


def solve_cg(H, l, x, b, accuracy):
    """solveCG: Jacobi-preconditioned CG in fp64 on level l -> x (fp32), iterations.  Vectors are held at the active vertices
    only (the reference skips the others in every loop, and their p and z stay 0)."""
    av, idx, coef, ok = _cg_terms(H, l)
    acc = f64(f32(accuracy))
    diag = H.A[l][0][av].astype(f64)
    full = np.zeros(x.size, f64)
    head = np.zeros((1, av.size), f64)

    def apply(vec):
        """the terms one after the other, starting from +0 (absent terms add +0, which changes no sum that started at +0)"""
        full[av] = vec
        return np.cumsum(np.concatenate((head, np.where(ok, coef * full[idx], 0.0))), axis=0)[-1]

    full[:] = x
    xd = x.astype(f64)[av]
    r = b.astype(f64)[av] - np.cumsum(np.concatenate((head, np.where(ok, coef * full[idx], 0.0))), axis=0)[-1]
    full[:] = 0
    z = r / diag
    p = z.copy()
    initial = np.sqrt(_ordered_sum(r * r))
    alpha_top = _ordered_sum(r * z)
    it = 0
    with np.errstate(all="ignore"):
        while it < 10000 and initial > 1e-12:
            z = apply(p)
            alpha = alpha_top / _ordered_sum(p * z)
            xd = xd + alpha * p
            r = r - alpha * z
            res = np.sqrt(_ordered_sum(r * r))
            z = r / diag
            alpha_top_new = _ordered_sum(r * z)
            if res / initial < acc:
                break
            beta = alpha_top_new / alpha_top
            alpha_top = alpha_top_new
            p = z + beta * p
            it += 1
    out = x.copy()
    out[av] = xd.astype(f32)
    return out, it


def vcycle(H, rhs, accuracy=1e-8, trace=None):
    """setRhs + doVCycle with a zero initial guess and (1, 1) smoothing on a hierarchy whose vectors are all zero -> dict
    b, x (lists per level, as they stand after the cycle), result (= x[0]), cg_iters.  trace, if a list, receives
    (name, level, array) after every pass in the order of the down sweep and then the up sweep."""
    n = [s[0] * s[1] * s[2] for s in H.sizes]
    b = [np.zeros(k, f32) for k in n]
    x = [np.zeros(k, f32) for k in n]
    r = [np.zeros(k, f32) for k in n]
    rhs = np.asarray(rhs, f32).reshape(n[0])
    b[0] = np.where(H.t[0] == TRIVIAL, rhs * TRIVIAL_SCALE, rhs)
    last = H.nl - 1

    def note(name, l, a):
        if trace is not None:
            trace.append((name, l, a.copy()))

    for l in range(last):
        x[l] = smooth(H, l, x[l], b[l], False)
        note("x after pre-smoothing", l, x[l])
        r[l] = residual(H, l, x[l], b[l], r[l])
        b[l + 1] = restrict(H, l + 1, r[l], b[l + 1])
        x[l + 1] = np.zeros(n[l + 1], f32)
        note("b after restriction", l + 1, b[l + 1])
    x[last], iters = solve_cg(H, last, x[last], b[last], accuracy)
    note("x after the coarsest CG", last, x[last])
    for l in range(last - 1, -1, -1):
        x[l] = interp_add(H, l, x[l + 1], x[l])
        x[l] = smooth(H, l, x[l], b[l], True)
        note("x after post-smoothing", l, x[l])
    return dict(b=b, x=x, result=x[0].reshape(H.sizes[0][2], H.sizes[0][1], H.sizes[0][0]), cg_iters=iters)
