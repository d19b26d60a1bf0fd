"""A plain numpy statement of the reference's GridMg in its 2-D mode (source/multigrid.cpp with mIs3D == false: a 5-point stencil
in 3 stored entries on level 0, a 9-point stencil in 5 stored entries above it, two colours of the smoother on level 0 and four
above), in its types and summation orders.  tests/test_mg2d_model.py ties it to the recorded fixture tests/golden/mg2d.npz,
tests/test_gpu_mg2d.py compares the HIP library with it level by level.

The 2-D mode is the 3-D algorithm on a grid with one plane: every loop of the reference over z runs once (mStencilMin/Max.z = 0),
and what the 3-D statement tests/mg_model.py does with the z neighbours of a vertex it skips on a grid with sz == 1, because they
are outside the grid.  Term for term:
    sizes          (s + 2) / 2 gives 1 for z = 1, and "every axis <= 5" holds for z
    activation     analyzeStencil sets A[3] = A[6] = 0: the z entries of an all-zero Ak plane
    selection      the keys 1 << (odd x + odd y) stay within 1..4 (the reference sizes its heap with 5 keys there, :531; the
                   lists of keys that never occur stay empty, so a larger key array pops in the same order)
    operators      entry sc of the 9-point stencil is entry 9 + sc of the 27-point one, stored at sc - 4 = (9 + sc) - 13; the
                   fine entries likewise; the loop order U, N, W is (y, x) in both
    rows           s = 0..8 in (y, x) order are the entries 9..17 of the 27-point row, in the same order
    colours        level 0: {(0,0), (1,1)} then {(1,0), (0,1)} is the parity of x + y (+ z = 0); above: the four offsets
                   (c & 1, c >> 1) are the first four of the eight, and the other four have no vertex
So this module states the 2-D hierarchy by handing (sx, sy, 1) and a zero Ak to mg_model and cutting the planes that a 2-D
operator does not store (asserting that they are zero).  What it adds of its own: the literal serial colour sweep of
knSmoothColor in 2-D (smooth_serial, which test_mg2d_model.py holds against the vectorised one), and the generation of the
level-1 paths in the reference's loop order (paths_unsorted: the count and the sc range; their order after std::sort belongs
to the sort and is recorded in the fixture).

THE LEVEL-1 OPERATOR.  As in mg_model: the model owns it where the sums do not depend on the order of the sorted paths (integer
systems); for the coefficient systems the recorded operator goes in (A1_patch, as the fixture stores it).

Layout: vertex v = x + sx * y; operators are (3, n) on level 0 (A0, Ai, Aj) and (5, n) above (plane s = entry 4 + s of the 9-point
stencil).  Types: 0 inactive, 1 active, 2 active trivial."""
import numpy as np

import mg_model as M3

f32, f64 = np.float32, np.float64
INACTIVE, ACTIVE, TRIVIAL = M3.INACTIVE, M3.ACTIVE, M3.TRIVIAL


def dims3(dims):
    assert len(dims) == 2 or dims[2] == 1, dims
    return (int(dims[0]), int(dims[1]), 1)


def level_sizes(dims):
    """GridMg::GridMg with gridSize.z == 1: ((sx + 2) / 2, (sy + 2) / 2, 1) until both axes are <= 5 or the level has <= 1000 vertices"""
    sizes = [dims3(dims)]
    while not ((sizes[-1][0] <= 5 and sizes[-1][1] <= 5) or sizes[-1][0] * sizes[-1][1] <= 1000):
        sizes.append(((sizes[-1][0] + 2) // 2, (sizes[-1][1] + 2) // 2, 1))
    return sizes


def planes(H, l):
    """the operator of level l as a 2-D hierarchy stores it: 3 planes on level 0, 5 above"""
    keep = 3 if l == 0 else 5
    assert not H.A[l][keep:].any(), "a plane that couples to z is not zero on level %d" % l
    return H.A[l][:keep]


def setup(dims, A, A1_patch=None, types=None):
    """GridMg::setA on the three planes A0, Ai, Aj.  A1_patch: the recorded level-1 operator of a system whose level-1 sums are not
    exact, as (flat indices into (5, n1), values) of the entries in which it differs from the generic-order fp32 sums.  A flat
    index into (5, n1) is the same flat index into mg_model's (14, n1).  -> mg_model's Hierarchy with A2[l] = planes(H, l)"""
    d = dims3(dims)
    n = d[0] * d[1]
    A = [np.asarray(a, f32).reshape(n) for a in A]
    assert len(A) == 3
    H = M3.setup(d, A + [np.zeros(n, f32)], A1_patch=A1_patch, types=types)
    assert H.sizes == level_sizes(d)
    H.A2 = [planes(H, l) for l in range(H.nl)]
    return H


def vcycle(H, rhs, accuracy=1e-8, trace=None):
    return M3.vcycle(H, rhs, accuracy, trace)


# ---------------------------------------------------------------------------------------------------------
# the literal serial sweep
# ---------------------------------------------------------------------------------------------------------
COLOURS0 = [[(0, 0), (1, 1)], [(1, 0), (0, 1)]]          # smoothGS, multigrid.cpp:724
COLOURS = [[(0, 0)], [(1, 0)], [(0, 1)], [(1, 1)]]       # :725


def smooth_serial(H, l, x, b, reverse):
    """knSmoothColor / smoothGS in 2-D as the reference writes it: colour by colour, block by block, offset by offset, one vertex at
    a time in place; fp32, one rounding per operation"""
    sx, sy, _ = H.sizes[l]
    t, A = H.t[l], H.A2[l]
    x = x.copy()
    cols = COLOURS0 if l == 0 else COLOURS
    bx, by = (sx + 1) // 2, (sy + 1) // 2
    for colour in (reversed(cols) if reverse else cols):
        for blk in range(bx * by):
            for ox, oy in colour:
                X, Y = 2 * (blk % bx) + ox, 2 * (blk // bx) + oy
                if X >= sx or Y >= sy:
                    continue
                v = X + sx * Y
                if t[v] == INACTIVE:
                    continue
                s = f32(b[v])
                if l == 0:
                    for d, (c, dim, pitch) in enumerate(((X, sx, 1), (Y, sy, sx))):
                        if c > 0:
                            s = f32(s - f32(A[d + 1][v - pitch] * x[v - pitch]))
                        if c < dim - 1:
                            s = f32(s - f32(A[d + 1][v] * x[v + pitch]))
                else:
                    si = 0
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            nx, ny = X + dx, Y + dy
                            if si != 4 and 0 <= nx < sx and 0 <= ny < sy and t[nx + sx * ny] != INACTIVE:
                                nn = nx + sx * ny
                                a = A[4 - si][nn] if si < 5 else A[si - 4][v]
                                s = f32(s - f32(a * x[nn]))
                            si += 1
                with np.errstate(divide="ignore", invalid="ignore"):
                    x[v] = f32(s) / f32(A[0][v])
    return x


# ---------------------------------------------------------------------------------------------------------
# the level-1 paths
# ---------------------------------------------------------------------------------------------------------
def paths_unsorted():
    """the coarsening paths of multigrid.cpp:286-312 with mDim = 2 in the order the reference generates them, as rows
    (N.x, N.y, U.x, U.y, W.x, W.y, sc, sf, inUStencil, rw, iw)"""
    p5 = [(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)]
    out = []
    for uy in (1, 2, 3):
        for ux in (1, 2, 3):
            for i, (ox, oy) in enumerate(p5):
                wx, wy = ux + ox, uy + oy
                for ny in range(wy // 2, (wy + 1) // 2 + 1):
                    for nx in range(wx // 2, (wx + 1) // 2 + 1):
                        s = nx + 3 * ny + 9
                        if s >= 13:
                            out.append((nx - 1, ny - 1, ux - 2, uy - 2, wx - 2, wy - 2, s - 13, (i + 1) // 2, int(i % 2 == 0),
                                        1.0 / (1 << ((ux % 2) + (uy % 2))), 1.0 / (1 << ((wx % 2) + (wy % 2)))))
    return out


def path_sort_key(p):
    """pathLess, multigrid.cpp:314-317: by sc, then by the position of U (ties are left to std::sort)"""
    return (p[6], (p[2] + 1) + 3 * (p[3] + 1))
