"""-m gpu: the base kernels (advect.hip, flip.hip, glue.hip, surface.hip, noise.hip, turbulence.hip) at the branches and launch
edges that the seeded inputs of test_gpu_parity.py do not reach.  Every comparison is HIP against the oracle, bit for bit, through
the package, on the inputs of the edge section of cases.py; each test first asserts, with numpy predicates on the inputs, that the
branches it was planted for are reached (tests/test_base_edges_inputs.py does the same on the CPU).

  test_flag_at_clamps_*        flag_at's plane clamp and flat-index clamp (particles beside the domain, nearest cell obstacle / fluid),
                               PNEW + skipNew, ptype & exclude and the excluded-particle arm of the clamp in k_advect_in_grid
  test_zmarch_depths           k_semi_lagrange_zmarch at depths 2, 3, 4, 5, 6, 8 and planes so small that a block spans z-groups
  test_flip_transfers_*        y < 0 and z < 0 in build_index_shift
  test_surface_pieces_*        norm / normalize3 at exactly 0 and exactly 1, getGradient's k clamps, projectOutOfBnd's inside arms and absent planes,
                               ptype & exclude in every ptsplugin and among indexed particles, markIsolatedFluidCell by direction
  test_mark_fluid_cells_*      ptype / exclude skip, particles outside the grid, fluid -> empty reset, both arms of the phiObs tests
  test_turbulence_*            the noise clamp (both bounds), weight grid of the same / another resolution, fluid cells with EMPTY
                               lower neighbours and a curl of norm exactly 1 in vorticityConfinement
  test_outflow_*               applyOutflowBC with 4 dt > 1 and 4 dt < 1, fluid below and above the outflow cells
  test_advect_from_poisoned_*  advectSemiLagrange's scratch grids taken from a pool full of NaN"""
import numpy as np
import pytest

import cases
import util
from util import assert_bitexact

pytestmark = pytest.mark.gpu


def _on_oracle(fn):
    from mantaflow_amd import _lib
    _lib.use_library(util.build_oracle(), "cpu")
    try:
        return fn()
    finally:
        _lib.reset()


def _same(a, b, what):
    if isinstance(b, dict):
        assert set(a) == set(b)
        for k in b:
            if isinstance(b[k], np.ndarray):
                assert_bitexact(a[k], b[k], "%s %s" % (what, k))
    else:
        assert_bitexact(a, b, what)


# ---- the two families that index near the end of an array ------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dims", cases.EDGE_DIMS)
def test_flag_at_clamps_advect_in_grid(hip_backend, dims, mode):
    I = cases.advect_parts_edge_inputs(dims, 19)
    cases.assert_reach(cases.advect_parts_edge_reach(dims, I), "advect_parts_edge_inputs%s" % (dims,))
    for m, dele, stop, skip in cases.ADVECT_PARTS_MODES:
        if m != mode:
            continue
        what = "advectInGrid mode %d deleteInObstacle %s stopInObstacle %s skipNew %s" % (mode, dele, stop, skip)
        p, f = cases.run_advect_parts_edge(dims, I, mode, dele, stop, skip)
        po, fo = _on_oracle(lambda: cases.run_advect_parts_edge(dims, I, mode, dele, stop, skip))
        assert_bitexact(f, fo, what + ": particle flags")
        assert_bitexact(p, po, what + ": positions")
        if not dele and stop:
            cases.check_planted_against_model(I, p, f)      # the flag of the nearest cell decides


@pytest.mark.parametrize("dims", cases.ZMARCH_DIMS)
def test_zmarch_depths(hip_backend, dims):
    """Real and Vec3 grids, order 1 and 2, orderTrace 1, linear: the z-marching kernel, its scratch grids taken from a poisoned pool
    so that the boundary zeros it writes count.  tools/zmarch_bounds.c ran the oracle on every shape of cases.ZMARCH_DIMS under
    AddressSanitizer / UBSan: none reads or writes out of bounds, none was dropped."""
    sx, sy, sz = dims
    flags, vel = cases.advect_inputs(dims, 9, vmax=2.5)
    border = np.ones((sz, sy, sx), bool)
    border[1:-1, 1:-1, 1:-1] = False
    for kind in (0, 1):
        field = util.rand_real((sz, sy, sx), 10) if kind == 0 else util.rand_vel(sx, sy, sz, 10)
        for order in (1, 2):
            what = "advectSemiLagrange %s kind %d order %d" % (dims, kind, order)
            got, seen = cases.run_advect_poisoned(dims, 0.9, flags, vel, field, kind, order=order)
            cases.check_poison_used(seen, kind, order)
            want = _on_oracle(lambda: cases.run_advect_pkg(dims, 0.9, flags, vel, field, kind, order=order))
            assert not np.isnan(got).any(), what
            assert_bitexact(got, want, what)
            assert (got[..., border] == 0).all(), what


# ---- the rest ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", cases.EDGE_DIMS)
def test_flip_transfers_beside_low_faces(hip_backend, dims):
    I = cases.flip_edge_inputs(dims, 14)
    cases.assert_reach(cases.flip_edge_reach(dims, I), "flip_edge_inputs%s" % (dims,))
    run = lambda: cases.run_flip_pkg(dims, I["flags"], I["vel"], I["velOld"], I["pos"], I["pflag"], I["pvel"], I["ptype"], 4)
    _same(run(), _on_oracle(run), "flip transfers")


@pytest.mark.parametrize("dims", cases.EDGE_DIMS)
def test_surface_pieces_edges(hip_backend, dims):
    I = cases.surface_edge_inputs(dims, 51)
    cases.assert_reach(cases.surface_edge_reach(dims, I), "surface_edge_inputs%s" % (dims,))
    run = lambda: dict(cases.run_surface_pkg(dims, I), **cases.run_project_pkg(dims, I))
    _same(run(), _on_oracle(run), "surface pieces")


@pytest.mark.parametrize("dims", cases.EDGE_DIMS)
def test_mark_fluid_cells_edges(hip_backend, dims):
    I = cases.markfluid_edge_inputs(dims, 31)
    cases.assert_reach(cases.markfluid_edge_reach(dims, I), "markfluid_edge_inputs%s" % (dims,))
    run = lambda: cases.run_markfluid_pkg(dims, I)
    _same(run(), _on_oracle(run), "markFluidCells")


@pytest.mark.parametrize("dims,small", [((20, 14, 12), (10, 7, 6)), (cases.SIZE_2D, (12, 9, 1)), ((17, 11, 9), (9, 6, 5))])
def test_turbulence_edges(hip_backend, dims, small):
    I = cases.turb_edge_inputs(dims, small, 91)
    cases.assert_reach(cases.turb_edge_reach(dims, I), "turb_edge_inputs%s" % (dims,))
    cases.assert_reach(_on_oracle(lambda: cases.turb_clamp_reach(cases.run_turb_edge_pkg, dims, I)), "noise clamp %s" % (dims,))
    run = lambda: cases.run_turb_edge_pkg(dims, I)
    _same(run(), _on_oracle(run), "turbulence pieces")


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("dims", [(14, 12, 10), cases.SIZE_2D])
def test_outflow_timestep_above_one(hip_backend, dims, order):
    """applyOutflowBC at dt = 0.9: 4 dt > 1, timeStep = 3.6"""
    sx, sy, sz = dims
    flags, vel = cases.advect_inputs(dims, 9, vmax=2.5, outflow=True)
    assert ((flags & util.OUTFLOW) != 0).sum() >= 8 and 4 * 0.9 > 1
    field = util.rand_vel(sx, sy, sz, 10)
    run = lambda: cases.run_advect_pkg(dims, 0.9, flags, vel, field, 2, order=order, strength=0.8 if order == 2 else 1.0)
    _same(run(), _on_oracle(run), "MAC advection with outflow, order %d" % order)


@pytest.mark.parametrize("dt", cases.OUTFLOW_DTS)
@pytest.mark.parametrize("dims", [(14, 12, 10), cases.SIZE_2D])
def test_outflow_both_sides_both_timesteps(hip_backend, dims, dt):
    """outflow cells with their fluid on the low and on the high side, bulk velocities above 1, timeStep = 4 dt and timeStep = 1"""
    flags, vel, field = cases.outflow_edge_inputs(dims, 9)
    cases.assert_reach(cases.outflow_edge_reach(dims, flags), "outflow_edge_inputs%s" % (dims,))
    for order in (1, 2):
        run = lambda: cases.run_advect_pkg(dims, dt, flags, vel, field, 2, order=order, strength=0.8 if order == 2 else 1.0)
        _same(run(), _on_oracle(run), "MAC advection with outflow on both sides, dt %g order %d" % (dt, order))


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("dims", [(14, 12, 10), cases.SIZE_2D])
def test_advect_from_poisoned_pool(hip_backend, dims, kind):
    """fwd, bwd and newg come from the pool without the clear: HIP from a pool full of NaN equals the oracle from a fresh one"""
    sx, sy, sz = dims
    flags, vel = cases.advect_inputs(dims, 9, vmax=2.5, outflow=(kind == 2))
    field = util.rand_real((sz, sy, sx), 10) if kind == 0 else util.rand_vel(sx, sy, sz, 10)
    for k, order, cm, ot, os_ in cases.ADVECT_POISON_CASES:
        if k != kind:
            continue
        what = "advectSemiLagrange from a poisoned pool: kind %d order %d clampMode %d orderTrace %d orderSpace %d" % (kind, order, cm, ot, os_)
        kw = dict(order=order, clampMode=cm, orderTrace=ot, orderSpace=os_, strength=0.8 if order == 2 else 1.0)
        got, seen = cases.run_advect_poisoned(dims, 0.9, flags, vel, field, kind, **kw)
        cases.check_poison_used(seen, kind, order)
        want = _on_oracle(lambda: cases.run_advect_pkg(dims, 0.9, flags, vel, field, kind, **kw))
        assert not np.isnan(got).any(), what
        assert_bitexact(got, want, what)
