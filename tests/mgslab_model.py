"""The z-slab schedule of the multigrid V-cycle (mantaflow_amd/slab.py: SlabMG.vcycle, include/open/manta_hip_mgslab.h), restated
on the numpy model of the hierarchy (tests/mg_model.py) with explicit per-rank copies: level 0 is cut along z, the levels >= 1 are
replicated.

Every rank holds its own whole-domain copies of x, b and r of level 0 and of b of level 1.  They start as NaN everywhere, and a
rank's ghost planes are poisoned with NaN again before each exchange fills them: a pass that reads a plane the schedule did not
bring there puts NaN into the result.  The passes are those of mg_model, masked to a range of planes.

  1. set-rhs on the owned planes [z0, z1); x = 0 on the owned and the ghost planes z0 - 1, z1
  2. colour 0 on the owned planes; exchange x; colour 1; exchange x
  3. residual on the owned planes; exchange r
  4. restriction into the owned coarse planes (coarse plane K belongs to the owner of fine plane min(2K, NZ - 1));
     all-gather of b of level 1, every plane copied from its owner
  5. the levels 1 .. L-1 of the undivided V-cycle, replicated
  6. interpolate-and-add on the owned and the ghost planes
  7. colour 1 on the owned planes; exchange x; colour 0
  8. the result is x on the owned planes
"""
import numpy as np

import mg_model as M

f32 = np.float32


def coarse_planes(z0, z1, NZ):
    """the coarse planes [K0, K1) owned by the owner of the fine planes [z0, z1)"""
    return (z0 + 1) // 2, ((NZ + 2) // 2 if z1 >= NZ else (z1 + 1) // 2)


def ranges_of(NZ, cuts):
    """cuts: the interior boundaries, increasing -> [(z0, z1)] per rank"""
    edges = [0] + list(cuts) + [NZ]
    assert all(a < b for a, b in zip(edges, edges[1:])), "every rank owns at least one plane"
    return list(zip(edges, edges[1:]))


def _planes(size, z0, z1):
    """mask of the vertices of a level on the planes [z0, z1) clipped to the level"""
    Z = M._coords(size)[2]
    return (Z >= max(z0, 0)) & (Z < min(z1, size[2]))


def smooth_colour(H, x, b, colour, mask):
    """one colour of knSmoothColor on level 0, on the vertices of `mask`"""
    size, t, A = H.sizes[0], H.t[0], H.A[0]
    X, Y, Z = M._coords(size)
    mine = (((X + Y + Z) & 1) == colour) & (t != M.INACTIVE) & mask
    s = M._row0(size, A, x, b)
    with np.errstate(all="ignore"):
        return np.where(mine, s / A[0], x)


def coarse_cycle(H, b1, accuracy):
    """the levels 1 .. L-1 of mg_model.vcycle, down and up, from b of level 1 and zero vectors -> x and b per level (index 0 unused)"""
    n = [s[0] * s[1] * s[2] for s in H.sizes]
    last = H.nl - 1
    b = [None] + [np.zeros(k, f32) for k in n[1:]]
    x = [None] + [np.zeros(k, f32) for k in n[1:]]
    r = [None] + [np.zeros(k, f32) for k in n[1:]]
    b[1] = b1
    for l in range(1, last):
        x[l] = M.smooth(H, l, x[l], b[l], False)
        r[l] = M.residual(H, l, x[l], b[l], r[l])
        b[l + 1] = M.restrict(H, l + 1, r[l], b[l + 1])
        x[l + 1] = np.zeros(n[l + 1], f32)
    x[last], iters = M.solve_cg(H, last, x[last], b[last], accuracy)
    for l in range(last - 1, 0, -1):
        x[l] = M.interp_add(H, l, x[l + 1], x[l])
        x[l] = M.smooth(H, l, x[l], b[l], True)
    return x, b, iters


def vcycle(H, rhs, ranges, accuracy=1e-8, leave_out=None):
    """the cut V-cycle on a hierarchy of at least two levels -> dict result (the owned planes of every rank put together, as
    mg_model.vcycle's), x, b (per level; level 0 assembled from the owners), exchanges, gathers (counts per V-cycle).
    leave_out: the number (0..3) of an exchange that only poisons the ghost planes and brings nothing -- to show that it is needed"""
    assert H.nl >= 2
    size0, size1 = H.sizes[0], H.sizes[1]
    NZ = size0[2]
    n0, n1 = size0[0] * size0[1] * size0[2], size1[0] * size1[1] * size1[2]
    P = len(ranges)
    rhs = np.asarray(rhs, f32).reshape(n0)
    nan = f32(np.nan)
    x = [np.full(n0, nan, f32) for _ in range(P)]
    b = [np.full(n0, nan, f32) for _ in range(P)]
    r = [np.full(n0, nan, f32) for _ in range(P)]
    b1 = [np.full(n1, nan, f32) for _ in range(P)]
    own = [_planes(size0, z0, z1) for z0, z1 in ranges]
    ghost = [_planes(size0, z0 - 1, z0) | _planes(size0, z1, z1 + 1) for z0, z1 in ranges]
    owner = np.full(n0, -1)
    for q in range(P):
        owner[own[q]] = q
    assert (owner >= 0).all()
    counts = dict(exchanges=0, gathers=0)

    def exchange(vecs):
        """every rank's ghost planes from their owners; poisoned first"""
        src = [v.copy() for v in vecs]
        for q in range(P):
            vecs[q][ghost[q]] = nan
            for p in range(P if counts["exchanges"] != leave_out else 0):
                m = ghost[q] & own[p]
                vecs[q][m] = src[p][m]
        counts["exchanges"] += 1

    act0 = H.t[0] != M.INACTIVE
    with np.errstate(invalid="ignore"):
        # 1
        for q in range(P):
            b[q] = np.where(own[q], np.where(H.t[0] == M.TRIVIAL, rhs * M.TRIVIAL_SCALE, rhs), b[q])
            x[q] = np.where(own[q] | ghost[q], f32(0), x[q])
        # 2
        for q in range(P):
            x[q] = smooth_colour(H, x[q], b[q], 0, own[q])
        exchange(x)
        for q in range(P):
            x[q] = smooth_colour(H, x[q], b[q], 1, own[q])
        exchange(x)
        # 3
        for q in range(P):
            r[q] = np.where(own[q] & act0, M._row0(size0, H.A[0], x[q], b[q], diag=True), r[q])
        exchange(r)
        # 4
        cown = [_planes(size1, *coarse_planes(z0, z1, NZ)) for z0, z1 in ranges]
        cowner = np.full(n1, -1)
        for q in range(P):
            assert (cowner[cown[q]] == -1).all(), "a coarse plane with two owners"
            cowner[cown[q]] = q
            b1[q] = np.where(cown[q], M.restrict(H, 1, r[q], np.zeros(n1, f32)), b1[q])
        assert (cowner >= 0).all(), "a coarse plane without an owner"
        whole = np.zeros(n1, f32)
        for q in range(P):
            whole[cown[q]] = b1[q][cown[q]]           # copied, never summed
        b1 = [whole.copy() for _ in range(P)]
        counts["gathers"] += 1
        # 5: replicated -- the same input on every rank, so once
        xc, bc, iters = coarse_cycle(H, b1[0], accuracy)
        # 6
        for q in range(P):
            x[q] = np.where(own[q] | ghost[q], M.interp_add(H, 0, xc[1], x[q]), x[q])
        # 7
        for q in range(P):
            x[q] = smooth_colour(H, x[q], b[q], 1, own[q])
        exchange(x)
        for q in range(P):
            x[q] = smooth_colour(H, x[q], b[q], 0, own[q])
    # 8
    x0, b0 = np.zeros(n0, f32), np.zeros(n0, f32)
    for q in range(P):
        x0[own[q]] = x[q][own[q]]
        b0[own[q]] = b[q][own[q]]
    return dict(result=x0.reshape(size0[2], size0[1], size0[0]), x=[x0] + xc[1:], b=[b0] + bc[1:], cg_iters=iters, **counts)
