"""The numpy statement of fluid guiding (tests/guiding_model.py) against the reference's recorded results (tests/golden/guiding.npz),
bit for bit, without a GPU: the Gaussian weights for radii 0-16, and every stage of the box case taken apart -- Q, invA, then per
iteration x, z before the solve, y and the two stop scalars, the recorded z after the solve being fed in, so no pressure solve runs
here."""
import numpy as np
import pytest

import guiding_model as M
from util import assert_bitexact


@pytest.fixture(scope="module")
def G():
    return M.golden()


@pytest.mark.parametrize("radius", list(M.RADII))
def test_weights(G, radius):
    w = M.weights(radius)
    assert w.dtype == np.float32 and len(w) == 2 * radius + 1
    assert_bitexact(w, G["weights/%d" % radius], "weights of radius %d" % radius)
    assert (w > 0).all() and abs(float(w.astype(np.float64).sum()) - 1) < 1e-6     # none of these is small enough to be dropped


def test_sparse_matrix_drops_small_entries():
    """a weight at or below 1e-6 is never stored by the reference's sparse matrix and reads back as 0"""
    assert M._sparse(1e-6) == 0 and M._sparse(-1e-6) == 0 and M._sparse(1.0000001e-6 * 1.01) != 0 and M._sparse(0.25) == np.float32(0.25)


def test_blur_skips_taps_outside_and_keeps_obstacle_neighbours():
    """the properties of the blur the model must have before it is a yardstick for the kernels: no renormalisation at the sides,
    radius 0 is a multiplication by the single weight, obstacle cells and their upper x / y / z neighbours keep their values"""
    rng = np.random.RandomState(3)
    a = rng.uniform(-1, 1, (3, 4, 5, 3)).astype(np.float32)
    free = np.full((3, 4, 5), M.FLUID, np.int32)
    w0 = M.weights(0)
    assert_bitexact(M.blur(a, free, w0, True), ((a * w0[0]) * w0[0]) * w0[0], "radius 0")
    ones = np.ones((1, 6, 7, 3), np.float32)
    b = M.blur(ones, free[:1, :1, :1].repeat(6, 1).repeat(7, 2), M.weights(2), False)
    assert b[0, 3, 3, 0] > b[0, 0, 3, 0] > b[0, 0, 0, 0] and b[0, 3, 3, 0] <= 1
    fl = free.copy()
    fl[1, 2, 3] = M.OBSTACLE
    c = M.blur(a, fl, M.weights(1), True, times=2)
    for (k, j, i) in ((1, 2, 3), (1, 2, 4), (1, 3, 3), (2, 2, 3)):
        assert_bitexact(c[k, j, i], a[k, j, i], "kept cell")
    assert not np.array_equal(c[1, 2, 2], a[1, 2, 2]) and not np.array_equal(c[0, 2, 3], a[0, 2, 3])
    fl2 = free[:1].copy()
    fl2[0, 2, 3] = M.OBSTACLE
    d = M.blur(a[:1], fl2, M.weights(1), False)            # 2-D: no z pass, no z neighbour
    assert_bitexact(d[0, 2, 4], a[0, 2, 4], "kept cell 2-D")


def test_staged_case(G):
    B = M.BOX
    I = M.box_inputs()
    flags, velC, is3d = I["flags"], I["vel"], True
    w = M.weights(B["blurRadius"])
    W = M.box_weight()
    sigma, tau, theta = B["sigma"], B["tau"], B["theta"]
    Q = M.precompute_q(I["velT"], velC, flags, w, sigma, is3d)
    assert_bitexact(Q, G["staged/Q"], "Q")
    invA = M.inv_a(W, sigma)
    assert_bitexact(invA, G["staged/invA"], "invA")
    x = y = z = np.zeros_like(velC)
    iters = len(G["staged/rnorm"])
    assert iters == M.BOX_RUNS["c_cap"]["maxIters"]
    for it in range(iters):
        x, z_pre = M.x_update(x, y, Q, invA, velC, z, flags, w, sigma, tau, is3d)
        assert_bitexact(x, G["staged/x"][it], "x, iteration %d" % it)
        assert_bitexact(z_pre, G["staged/z_pre"][it], "z before the solve, iteration %d" % it)
        z0, z = z, G["staged/z_post"][it]
        y, rnorm, zmax = M.post(z, z0, theta)
        assert_bitexact(y, G["staged/y"][it], "y, iteration %d" % it)
        assert rnorm == G["staged/rnorm"][it], (it, rnorm, G["staged/rnorm"][it])
        eps = M.eps_dual(M.BOX_RUNS["c_cap"]["epsAbs"], B["epsRel"], zmax, is3d)
        assert eps == G["staged/epsDual"][it], (it, eps, G["staged/epsDual"][it])
    assert_bitexact(z, G["c_cap/vel"], "the staged loop ends where the plugin does")


def test_recorded_conditions(G):
    """what the whole-plugin cases exist for, as the recorder asserted it on the reference"""
    assert G["c_cap/pd"][0] == M.BOX_RUNS["c_cap"]["maxIters"] - 1 and G["c_stop/pd"][0] == 1
    for name, cfg in M.LOOPS.items():
        pd = G[name + "/pd"]
        assert len(pd) == cfg["steps"] and all(0 < p < 199 for p in pd)
        assert len(G[name + "/cg"]) == int(pd.sum()) + len(pd)
