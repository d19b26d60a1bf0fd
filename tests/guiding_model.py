"""numpy fp32 statement of the arithmetic of source/plugin/fluidguiding.cpp around its inner pressure solve -- the Gaussian weights,
the separable blur with its obstacle restore, Q, invA, the x / z / y updates and the stop scalars -- plus the seeded inputs and the
case tables shared by tools/record_guiding.py (which records the reference's results into tests/golden/guiding.npz) and the tests.

Arrays are [z][y][x] (scalars) and [z][y][x][3] (MAC grids).  Every operation below is one fp32 rounding, in the order of the
reference's chain of grid methods."""
import math
import os

import numpy as np

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guiding.npz")
FLUID, OBSTACLE, EMPTY, OUTFLOW = 1, 2, 4, 16
RADII = range(17)


# ---- weights, fluidguiding.cpp:31-45 ------------------------------------------------------------------------------------------------
def _sparse(v):
    """Matrix::add_to_element (util/rcmatrix.h:186-187): |v| <= 1e-6f is never stored and reads back as 0"""
    v = f32(v)
    return v if abs(v) > f32(1e-6) else f32(0)


def weights(radius):
    """get1DGaussianBlurKernel(n, n), n = 2 radius + 1.  exp is the C library's float function: stated here as the double exp
    rounded once, which is what a correctly rounded expf returns."""
    n = 2 * radius + 1
    sigma = n
    G = np.zeros(n, f32)
    sumG = f32(0)
    for j in range(n):
        x = _sparse(-(n - 1) * 0.5)
        y = _sparse(j - (n - 1) * 0.5)
        arg = -(x * x + y * y) / f32(2 * sigma * sigma)
        e = f32(math.exp(float(arg)))
        G[j] = _sparse(1 / (2 * math.pi * sigma * sigma) * float(e))
        sumG = f32(sumG + G[j])
    k = 1.0 / float(sumG)
    for j in range(n):
        if G[j] != 0:
            G[j] = _sparse(float(G[j]) * k)
    return G


# ---- blur, :49-136 ------------------------------------------------------------------------------------------------------------------
def _pass(a, w, axis):
    """apply1DKernelDirX/Y/Z: axis 2 = x, 1 = y, 0 = z of [z][y][x][3]"""
    kn = len(w)
    r = kn // 2
    n = a.shape[axis]
    out = np.zeros_like(a)
    for m in range(kn):
        off = m - r                                   # tap = pos + off, skipped outside [0, n)
        lo, hi = max(0, -off), min(n, n - off)
        if lo >= hi:
            continue
        dst = [slice(None)] * 4
        src = [slice(None)] * 4
        dst[axis] = slice(lo, hi)
        src[axis] = slice(lo + off, hi + off)
        out[tuple(dst)] = out[tuple(dst)] + a[tuple(src)] * w[kn - 1 - m]
    return out


def keep_mask(flags, is3d):
    """cells that keep their value from before a blur: obstacles and cells whose lower x / y / (3-D) z neighbour is one"""
    ob = (flags & OBSTACLE) != 0
    keep = ob.copy()
    keep[:, :, 1:] |= ob[:, :, :-1]
    keep[:, 1:, :] |= ob[:, :-1, :]
    if is3d:
        keep[1:, :, :] |= ob[:-1, :, :]
    return keep


def blur(grid, flags, w, is3d, times=1):
    """applySeparableKernel2D / 3D, `times` in a row"""
    a = np.asarray(grid, f32)
    keep = keep_mask(flags, is3d)
    for _ in range(times):
        orig = a
        a = _pass(_pass(a, w, 2), w, 1)
        if is3d:
            a = _pass(a, w, 0)
        a = np.where(keep[..., None], orig, a)
    return a


# ---- precomputations and one iteration -------------------------------------------------------------------------------------------------
def inv_a(weight, sigma):
    """precomputeInvA, :254-263 (one value per cell)"""
    wv = np.asarray(weight, f32)
    val = f32(2) * wv * wv + f32(sigma)
    val = np.where(val.astype(np.float64) < 0.01, f32(0.01), val)
    return (1.0 / val.astype(np.float64)).astype(f32)


def precompute_q(velT, velC, flags, w, sigma, is3d):
    """:243-250"""
    q = np.asarray(velT, f32) - np.asarray(velC, f32)
    q = blur(q, flags, w, is3d, 2)
    q = q * f32(2)
    return q + f32(-f32(sigma)) * velC


def pre(x, y, Q, invA, sigma):
    sig = f32(sigma)
    inv_sigma = f32(1.0 / float(sig))
    v = x * inv_sigma
    v = v + y
    v = v * sig
    v = v + Q
    return v, v * invA[..., None]


def mid(x, y, xv, vn, invA, velC, z, sigma, tau):
    sig, a = f32(sigma), invA[..., None]
    b = vn * f32(2)
    b = b * a
    v = xv * a
    v = v - b
    v = v + velC
    v = v * f32(-sig)
    v = v + sig * y
    v = v + x
    return v, z + f32(-f32(tau)) * v


def max_abs(v):
    """Grid<Vec3>::getMaxAbs: sqrt of the largest x*x + y*y + z*z"""
    v = np.asarray(v, f32)
    return f32(np.sqrt(((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).max()))


def post(z, z0, theta):
    r = z - z0
    return r * f32(theta) + z, max_abs(r), max_abs(z)


def eps_dual(epsAbs, epsRel, zmax, is3d):
    """getEpsDual, :165-168: sqrt(3.0 or 2.0) * eps_abs in double, eps_rel * getMaxAbs() a Real product, the sum rounded to Real"""
    return f32(math.sqrt(3.0 if is3d else 2.0) * float(f32(epsAbs)) + float(f32(epsRel) * f32(zmax)))


def x_update(x, y, Q, invA, velC, z, flags, w, sigma, tau, is3d):
    """:323-331: returns the new x and z (before the solve)"""
    xv, vn = pre(x, y, Q, invA, sigma)
    return mid(x, y, xv, blur(vn, flags, w, is3d, 2), invA, velC, z, sigma, tau)


# ---- set-up plugins, :171-205 ----------------------------------------------------------------------------------------------------------
SETUP = {
    # getSpiralVelocity: dims, strength, with3D
    "spiral_2d": ((9, 7, 1), 1.5, False),
    "spiral_odd_centre": ((7, 5, 3), 0.3, True),         # odd sizes: the centre column has hypotenuse 0 and stays as it is
    "spiral_plane0": ((8, 6, 4), 2.0, False),            # with3D off on a 3-D grid: only plane 0 is written
    # setGradientYWeight: dims, minY, maxY, valAtMin, valAtMax
    "grad_ends": ((5, 9, 2), 2, 6, 1.0, 5.0),
    "grad_equal": ((5, 9, 2), 0, 4, 0.3, 0.3),
    "grad_past_top": ((4, 6, 1), 3, 11, 0.1, 0.7),
}


def setup_input(name):
    """the grid the set-up plugin is applied to (seeded, so untouched cells show)"""
    dims = SETUP[name][0]
    rng = np.random.RandomState(sum(map(ord, name)))
    shape = (dims[2], dims[1], dims[0])
    if name.startswith("spiral"):
        return rng.uniform(-1, 1, shape + (3,)).astype(f32)
    return rng.uniform(-1, 1, shape).astype(f32)


# ---- whole-plugin cases ------------------------------------------------------------------------------------------------------------------
PcMIC, PcMGStatic = 1, 3
BOX = dict(dims=(12, 10, 9), blurRadius=2, theta=0.7, tau=0.8, sigma=1.1, epsRel=1e-3, preconditioner=PcMIC)
BOX_RUNS = {"c_cap": dict(maxIters=3, epsAbs=1e-3), "c_stop": dict(maxIters=200, epsAbs=1e3)}
LOOPS = {
    # tools/tests/test_1050_guiding2d.py at res 40 = res0 40 x scale 1.  (At res0 20 x scale 2 the doubled target strength keeps the
    # closed domain's inner solves at their iteration cap and the reference's loop never meets its criterion.)
    "a": dict(dims=(40, 40, 1), steps=3, scale=1, blurRadius=2, tau=1.0, sigma=0.99 / 1.0, theta=1.0, epsRel=1e-3, epsAbs=1e-3,
              preconditioner=PcMIC),
    # scenes/guiding_3d02_high.py at res2 = 16, the target velocity from getSpiralVelocity(with3D=True) instead of the low-res files
    "b": dict(dims=(16, 32, 16), steps=2, factor=2, timestep=0.65, blurRadius=5, tau=0.58 / 2, sigma=2.44 / (0.58 / 2), theta=0.3,
              wScalar=2, epsRel=1e-3, epsAbs=1e-3, preconditioner=PcMGStatic),
}


def box_inputs():
    """case (c) and the staged case: a 12x10x9 domain with walls, an open top and an obstacle box inside, seeded velocities, a y-gradient weight
    (setGradientYWeight(W, 2, 7, 0.5, 3.0) on a grid of 1)"""
    sx, sy, sz = BOX["dims"]
    rng = np.random.RandomState(1050)
    flags = np.full((sz, sy, sx), FLUID, np.int32)
    flags[0], flags[-1], flags[:, 0], flags[:, -1], flags[:, :, 0], flags[:, :, -1] = (OBSTACLE,) * 6
    flags[1:-1, -1, 1:-1] = EMPTY                      # an open top: the inner solve has a Dirichlet side and is well posed
    flags[3:6, 4:7, 5:9] = OBSTACLE
    vel = rng.uniform(-1, 1, (sz, sy, sx, 3)).astype(f32)
    velT = rng.uniform(-1, 1, (sz, sy, sx, 3)).astype(f32)
    return dict(flags=flags, vel=vel, velT=velT, grad=(2, 7, 0.5, 3.0))


def box_weight():
    sx, sy, sz = BOX["dims"]
    W = np.ones((sz, sy, sx), f32)
    minY, maxY, vmin, vmax = box_inputs()["grad"]
    for j in range(minY, maxY + 1):
        ratio = f32(j - minY) / f32(maxY - minY)
        W[:, j, :] = f32(float(ratio * f32(vmax)) + (1.0 - float(ratio)) * float(f32(vmin)))
    return W


def golden():
    return np.load(GOLDEN)
