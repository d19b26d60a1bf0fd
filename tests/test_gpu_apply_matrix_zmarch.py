"""The z-marching packed ApplyMatrix (pressure.hip: k_apply_matrix_zmarch), alone and with its fused dot inside the PCG, on the HIP
library against the oracle.

ApplyMatrix is bit-exact, signed zeros included (bit patterns are compared).  The bars of the solves are those of
test_gpu_pcg_routes._agree: the same iteration count, dst within 1e-5 relative, resNorm and sigma within 1e-4.

The kernel serves whole packed 3-D grids.  mf_time_apply_matrix_packed (after mf_mic_init) and mf_apply_matrix (after mf_pack_matrix)
reach it at every shape here; mf_cg_solve reaches it where the system has no 8 x 8 bundle of rows without a fluid cell (a bundle made of
wall cells only -- sy % 8 == 1 or sz % 8 == 1 in a closed box -- puts the solve on the skip-map route, which keeps the tile kernel).  The solve shapes below hold both kinds."""
import ctypes

import numpy as np
import pytest

import cases
import util

pytestmark = pytest.mark.gpu

L = 16      # planes per segment (ZM_L in pressure.hip); a thread owns 2 rows (ZM_R)

# (8, 4, sz): every segment end, a last short segment, fewer planes than one segment
SHAPES = [(8, 4, sz) for sz in range(2, 2 * L + 2)] + [
    (4, 3, 5),        # a single quad, odd sy
    (8, 5, 3),        # the one-row last thread
    (264, 6, 5),      # 66 quads: a row crosses a wave boundary, the lane-edge fix-ups run mid-row
    (64, 33, 19),
]
_IDS = ["%dx%dx%d" % s for s in SHAPES]

_cache = {}


def _system(oracle, dims, a0_stream):
    """flags, matrix, src (30 % +0 and 20 % -0 planted, so that a rebuilt zero shows its sign) and the oracle's result, computed once
    per case.  A0 = 6.0 everywhere (the packed bytes carry the diagonal); with a0_stream A0 = 2.5 in 40 fluid cells (all of them where
    the shape has fewer), so that they cannot and the A0 array is read"""
    key = (dims, a0_stream)
    if key not in _cache:
        flags, A, src = cases.system_inputs(dims, 8)
        A = [a.copy() for a in A]
        rng = np.random.default_rng(31)
        fluid = np.argwhere((flags & util.FLUID) != 0)
        A[0][...] = np.float32(6.0)
        if a0_stream and len(fluid):
            for k, j, i in fluid[rng.choice(len(fluid), min(40, len(fluid)), replace=False)]:
                A[0][k, j, i] = np.float32(2.5)
        src = src.copy()
        src[rng.random(src.shape) < 0.3] = 0.0
        src[rng.random(src.shape) < 0.2] = -0.0
        want = cases.run_apply_matrix_impl(oracle, dims, flags, A, src)
        _cache[key] = (flags, A, src, want)
    return _cache[key]


def _same_bits(got, want, what):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s differs in %d cells, first at (k, j, i) = %s" % (what, bad.sum(), tuple(np.argwhere(bad)[0]))


@pytest.mark.parametrize("a0_stream", [False, True], ids=["nibble", "a0-stream"])
@pytest.mark.parametrize("dims", SHAPES, ids=_IDS)
def test_apply_matrix_after_mic_init(hip, oracle, dims, a0_stream):
    """the route of the PCG's ApplyMatrix: the packed bytes of mf_mic_init, through mf_time_apply_matrix_packed with one repetition"""
    sx, sy, sz = dims
    flags, A, src, want = _system(oracle, dims, a0_stream)
    f, s_, dA = hip.dev(flags), hip.dev(src), [hip.dev(a) for a in A]
    ap = hip.dev(np.zeros((sz, sy, sx), np.float32))
    dst = hip.dev(np.full((sz, sy, sx), 7.0, np.float32))
    hip.call("mf_mic_init", sx, sy, sz, f, ap, *dA, None)
    us = ctypes.c_double()
    hip.call("mf_time_apply_matrix_packed", sx, sy, sz, f, dst, s_, *dA, 1, ctypes.byref(us), None)
    hip.sync()
    _same_bits(hip.host(dst), want, "packed ApplyMatrix %s" % (dims,))


@pytest.mark.parametrize("a0_stream", [False, True], ids=["nibble", "a0-stream"])
@pytest.mark.parametrize("dims", SHAPES, ids=_IDS)
def test_apply_matrix_after_pack_matrix(hip, oracle, dims, a0_stream):
    """the packed bytes of mf_pack_matrix, through mf_apply_matrix"""
    sx, sy, sz = dims
    flags, A, src, want = _system(oracle, dims, a0_stream)
    f, s_, dA = hip.dev(flags), hip.dev(src), [hip.dev(a) for a in A]
    hip.call("mf_pack_matrix", sx, sy, sz, f, *dA, None)
    dst = hip.dev(np.full((sz, sy, sx), 7.0, np.float32))
    hip.call("mf_apply_matrix", sx, sy, sz, f, dst, s_, *dA, None)
    hip.sync()
    _same_bits(hip.host(dst), want, "mf_apply_matrix after mf_pack_matrix %s" % (dims,))


@pytest.mark.parametrize("dims", [(8, 4, 5), (264, 6, 5), (64, 33, 19)], ids=lambda d: "%dx%dx%d" % d)
def test_apply_matrix_fallback_when_not_packable(hip, oracle, dims):
    """a matrix that is not all 0 / -1 (Aj halved) after mf_pack_matrix: the general kernel, still the reference's bits"""
    sx, sy, sz = dims
    flags, A, src, _ = _system(oracle, dims, False)
    B = [a.copy() for a in A]
    B[2] *= np.float32(0.5)
    want = cases.run_apply_matrix_impl(oracle, dims, flags, B, src)
    f, s_, dB = hip.dev(flags), hip.dev(src), [hip.dev(b) for b in B]
    hip.call("mf_pack_matrix", sx, sy, sz, f, *dB, None)
    dst = hip.dev(np.full((sz, sy, sx), 7.0, np.float32))
    hip.call("mf_apply_matrix", sx, sy, sz, f, dst, s_, *dB, None)
    hip.sync()
    _same_bits(hip.host(dst), want, "scaled matrix after mf_pack_matrix %s" % (dims,))


# ---- the solve: ApplyMatrix with the fused dot (one fp64 partial per block, alpha = sigma / their sum) ----
TOL = 1e-5


def _close(a, b, what, tol=TOL):
    e = util.rel_err(a, b)
    assert e <= tol, "%s: relative error %g > %g" % (what, e, tol)


def _agree(got, want, what):
    assert got[1][0] == want[1][0], "%s: iterations %s vs %s" % (what, got[1], want[1])
    _close(got[0], want[0], what + ": dst")
    _close(got[1][1:], want[1][1:], what + ": resNorm/sigma", 1e-4)


# the first three as wall-only bundles decide (see the module text): skip-map route, z-march, skip-map route; the last two are the
# first and the third with one plane more, on the z-march route
SOLVE_SHAPES = [(16, 12, 9), (8, 8, 5), (64, 16, 2 * L + 1), (16, 12, 10), (64, 16, 2 * L + 2)]


def _solve_inputs(dims):
    flags, A, _ = cases.system_inputs(dims, 6)
    return flags, A, cases.cg_rhs(dims, flags, 6)


@pytest.mark.parametrize("dims", SOLVE_SHAPES, ids=lambda d: "%dx%dx%d" % d)
def test_cg_iterate_by_iterate(hip, oracle, dims):
    """a wrong alpha (or ApplyMatrix dot) that later iterations would correct shows in the iterate after k steps"""
    flags, A, rhs = _solve_inputs(dims)
    for k in range(1, 13):
        got = cases.run_cg_impl(hip, dims, flags, A, rhs, 2, 1e-7, k)
        want = cases.run_cg_impl(oracle, dims, flags, A, rhs, 2, 1e-7, k)
        _agree(got, want, "%s after %d iterations" % (dims, k))
        if want[1][0] < k:
            break
        assert got[1][0] == k


@pytest.mark.parametrize("dims", SOLVE_SHAPES, ids=lambda d: "%dx%dx%d" % d)
def test_cg_l2_norm(hip, oracle, dims):
    """useL2 = 1: the residual update's sum of squares instead of its min / max"""
    flags, A, rhs = _solve_inputs(dims)
    got = cases.run_cg_impl(hip, dims, flags, A, rhs, 2, 1e-7, 8, 1)
    want = cases.run_cg_impl(oracle, dims, flags, A, rhs, 2, 1e-7, 8, 1)
    _agree(got, want, "%s, L2 norm" % (dims,))


@pytest.mark.parametrize("dims", SOLVE_SHAPES, ids=lambda d: "%dx%dx%d" % d)
def test_cg_stops_at_max_iter(hip, oracle, dims):
    """accuracy out of reach, maxIter = 3: three iterations are counted and three pressure updates applied (iterations++ and xpending
    of the alpha step)"""
    flags, A, rhs = _solve_inputs(dims)
    got = cases.run_cg_impl(hip, dims, flags, A, rhs, 2, 1e-9, 3)
    want = cases.run_cg_impl(oracle, dims, flags, A, rhs, 2, 1e-9, 3)
    assert got[1][0] == 3, got[1]
    _agree(got, want, "%s, 3 iterations" % (dims,))


def _solve_keep(impl, dims, flags, A, rhs, maxIter):
    """mf_cg_solve(pc 2, accuracy 1e-3) -> (dst, iterations, diverged): dst is read back after a reported divergence as well"""
    sx, sy, sz = dims
    z = lambda: impl.dev(np.zeros((sz, sy, sx), np.float32))
    dst, residual, search, tmp, ap = z(), z(), z(), z(), z()
    out = (ctypes.c_float * 3)()
    diverged = False
    try:
        impl.call("mf_cg_solve", sx, sy, sz, impl.dev(flags), dst, impl.dev(rhs), residual, search, tmp, *[impl.dev(a) for a in A], ap, 2,
                  1e-3, maxIter, 0, out, None)
    except RuntimeError as e:
        if "diverged" not in str(e):
            raise
        diverged = True
    impl.sync()
    return impl.host(dst), int(out[0]), diverged


@pytest.mark.parametrize("dims", [(16, 16, 16), (16, 12, 10)], ids=lambda d: "%dx%dx%d" % d)
def test_cg_diverged_reports_like_reference(hip, oracle, dims):
    """test_gpu_parity.test_cg_diverged_reports_like_reference's input (closed box, random rhs scaled to 1e30: an inconsistent system)
    on the z-march route: divergence is reported where the oracle reports it, after the same number of iterations, and the iteration that
    diverged has finished its pressure update (the reference throws after it) -- dst is finite in the same cells and agrees there"""
    flags, A, _ = cases.system_inputs(dims, 4)
    rhs = cases.cg_rhs(dims, flags, 4) * 1e30
    got, it_g, div_g = _solve_keep(hip, dims, flags, A, rhs, 200)
    want, it_w, div_w = _solve_keep(oracle, dims, flags, A, rhs, 200)
    assert div_w, "the input is meant to diverge"
    assert div_g and it_g == it_w, ("diverged / iterations", div_g, it_g, div_w, it_w)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    if fin.any():
        _close(got[fin], want[fin], "dst after the diverged iteration")
