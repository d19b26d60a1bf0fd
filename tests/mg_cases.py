"""Inputs and runners shared by the multigrid tests (test_gpu_multigrid.py, test_multigrid_api.py, test_multigrid_golden.py).
Inputs are regenerated from tests/util.py, never stored: flags = util.make_flags(sx, sy, sz, seed=1, ...), vel =
util.smooth_vel(sx, sy, sz, 1) after setWallBcs (by the plain-C checker library, which the CPU suite pins to the reference)."""
import ctypes
import os

import numpy as np

import cases
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "multigrid.npz")
PcMIC, PcMGDynamic, PcMGStatic = 1, 2, 3

# kind -> (make_flags arguments, solvePressure arguments, ghost fluid?)
KINDS = {
    "box": (dict(obstacles=False), dict(cgAccuracy=1e-4, zeroPressureFixing=True), False),
    "obs": (dict(obstacles=True), dict(cgAccuracy=1e-3, zeroPressureFixing=True), False),
    "liq": (dict(obstacles=True, empty_top=True), dict(cgAccuracy=1e-5, useL2Norm=True), False),
    "gf": (dict(obstacles=True, empty_top=True), dict(cgAccuracy=1e-3), True),
}
SIZES = [(12, 10, 9), (24, 24, 24), (45, 33, 27), (61, 40, 24), (40, 52, 36), (52, 52, 52), (96, 64, 80), (128, 128, 128)]
STAGE_CASES = {"obs": (24, 24, 24), "liq": (45, 33, 27)}


def case_name(kind, dims):
    return "%s_%dx%dx%d" % ((kind,) + tuple(dims))


def wall_bcs(dims, flags, vel):
    """setWallBcs(flags, vel) on the host"""
    sx, sy, sz = dims
    impl = util.Impl("oracle")
    v = impl.dev(vel)
    impl.call("mf_set_wall_bcs", sx, sy, sz, impl.dev(flags), v, None, None)
    return impl.host(v).copy()


def inputs(kind, dims, vel_seed=1):
    sx, sy, sz = dims
    fkw, skw, ghost = KINDS[kind]
    flags = util.make_flags(sx, sy, sz, seed=1, **fkw)
    vel = wall_bcs(dims, flags, util.smooth_vel(sx, sy, sz, vel_seed))
    phi = None
    if ghost:
        zz, yy, xx = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
        phi = (yy - (2 * sy) // 3 + 0.3).astype(np.float32)
    return flags, vel, phi, dict(skw)


def run_ref(dims, flags, vel, phi, preconditioner=PcMGDynamic, fractions=None, cgAccuracy=1e-3, useL2Norm=False, zeroPressureFixing=False):
    """solvePressure of the compiled reference (a fresh FluidSolver per call, so a Dynamic hierarchy)"""
    sx, sy, sz = dims
    v = vel.copy()
    p = np.zeros((sz, sy, sx), np.float32)
    rr = np.zeros((sz, sy, sx), np.float32)
    util.refcall("ref_solve_pressure", sx, sy, sz, v, p, flags, ctypes.c_float(cgAccuracy), phi, None, fractions, None,
                 ctypes.c_float(1e-4), ctypes.c_float(1.5), 1, int(preconditioner), 0, int(useL2Norm), int(zeroPressureFixing), None,
                 ctypes.c_float(0.0), rr)
    return dict(vel=v, pressure=p, rhs=rr)


class PkgSolver(object):
    """one package solver with its grids, for sequences of solves on it"""

    def __init__(self, dims):
        from mantaflow_amd import core
        self.s = cases._mk_solver(dims)
        self.fl, self.v, self.p, self.rr = core.FlagGrid(self.s), core.MACGrid(self.s), core.Grid(self.s), core.Grid(self.s)
        self.core = core

    def solve(self, flags, vel, phi=None, fractions=None, **kw):
        from mantaflow_amd import plugins
        cases.soa_to_grid(self.fl, flags)
        cases.soa_to_grid(self.v, vel)
        ph = cases.soa_to_grid(self.core.LevelsetGrid(self.s), phi) if phi is not None else None
        fr = cases.soa_to_grid(self.core.MACGrid(self.s), fractions) if fractions is not None else None
        plugins.solvePressure(self.v, self.p, self.fl, phi=ph, fractions=fr, retRhs=self.rr, **kw)
        self.s.sync()
        return dict(vel=cases.grid_to_soa(self.v), pressure=cases.grid_to_soa(self.p), rhs=cases.grid_to_soa(self.rr),
                    iterations=plugins.lastCgStats()["iterations"])


def run_pkg(dims, flags, vel, phi=None, **kw):
    return PkgSolver(dims).solve(flags, vel, phi, **kw)


def stage_inputs(kind, dims):
    """the system of the stage tests: MakeLaplaceMatrix of the kind's flags (no pressure fixing) and a seeded rhs"""
    sx, sy, sz = dims
    flags = util.make_flags(sx, sy, sz, seed=1, **KINDS[kind][0])
    impl = util.Impl("oracle")
    A = cases.run_laplace_impl(impl, dims, flags, None)
    return flags, A, cases.cg_rhs(dims, flags, 7)


# Static / Dynamic semantics: three solves on one solver
STATIC_DIMS = (40, 52, 36)
STATIC_KW = dict(cgAccuracy=1e-3, zeroPressureFixing=True)


def static_sequence():
    """[(flags, vel, solvePressure arguments)]: (a) the obs flags, (b) the same flags with another velocity, (c) an obstacle blob
    added (the Static hierarchy of (a) then preconditions a matrix it was not built from)"""
    sx, sy, sz = STATIC_DIMS
    flags = util.make_flags(sx, sy, sz, seed=1, obstacles=True)
    flags2 = flags.copy()
    zz, yy, xx = np.ogrid[:sz, :sy, :sx]
    blob = (xx - 27) ** 2 + (yy - 14) ** 2 + (zz - 20) ** 2 <= 16
    flags2[blob & (flags2 == util.FLUID)] = util.OBS
    assert (flags2 != flags).sum() > 50
    out = []
    for f, seed in ((flags, 1), (flags, 2), (flags2, 3)):
        out.append((f, wall_bcs(STATIC_DIMS, f, util.smooth_vel(sx, sy, sz, seed)), dict(STATIC_KW)))
    return out


def mgsolve_step(step, prev_vel):
    """the four solves of the reference's tools/tests/test_0110_mgsolve.py at res 52 (flags: initDomain + fillGrid): Dynamic without
    wall conditions, Dynamic, Static, Static on the projected field of the third.  Its Box source (0.3..0.7, 0.4..0.8, 0.3..0.7 of
    the grid) is applied as: every component of the cells whose centre lies in the box is set to the value.
    -> flags, vel, preconditioner, solvePressure arguments"""
    res = 52
    dims = (res, res, res)
    flags = util.make_flags(res, res, res, seed=1, obstacles=False)
    c = np.arange(res) + 0.5
    inx = (c >= 0.3 * res) & (c <= 0.7 * res)
    iny = (c >= 0.4 * res) & (c <= 0.8 * res)
    box = inx[None, None, :] & iny[None, :, None] & inx[:, None, None]
    value = [(0.15, 0.3, 0.21), (1.5, 3.0, 2.1), (1.1, 2.0, -2.1), (-1.1, -2.0, 2.1)][step]
    vel = prev_vel.copy() if step == 3 else np.zeros((3, res, res, res), np.float32)
    for comp in range(3):
        vel[comp][box] = np.float32(value[comp])
    if step > 0:
        vel = wall_bcs(dims, flags, vel)
    return flags, vel, (PcMGDynamic if step < 2 else PcMGStatic), dict(cgAccuracy=1e-4, zeroPressureFixing=True)


FRACTIONS_DIMS = (48, 32, 32)


def fractions_inputs_model():
    """the obstacle loop's start by the numpy model: updateFractions(boundaryWidth=0), setObstacleFlags(fractions, boundaryWidth=1),
    fillGrid -> dims, flags, vel, fractions"""
    import obstacle_model as OM
    f, phi, vel = OM.loop_inputs(FRACTIONS_DIMS)
    fr = OM.update_fractions(f, phi, 0)
    f = OM.set_obstacle_flags(f, phi, fractions=fr, boundaryWidth=1)
    keep = (f & (OM.OBSTACLE | OM.INFLOW | OM.OUTFLOW | OM.OPEN)) != 0
    f = np.where(keep, f, (f & ~(OM.EMPTY | OM.FLUID)) | OM.FLUID).astype(np.int32)
    return FRACTIONS_DIMS, f, vel, fr
