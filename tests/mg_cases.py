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
LEVELS_GOLDEN = os.path.join(ROOT, "tests", "golden", "multigrid_levels.npz")      # recorded by tools/record_mg_levels.py
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

# Shapes that no size above reaches, with the level sizes GridMg must give them (coarsening stops at <= 1000 vertices, or when
# every dimension is <= 5): one-level hierarchies, the sizes around both stopping rules, coarsest levels of 729 and of exactly
# 1000 vertices, level 0 on either side of the library's 8192-vertex hand-over to its single-workgroup kernel, mixed parities,
# thin levels, and a single interior column.
EDGE_SHAPES = [
    ((10, 10, 10), [(10, 10, 10)]),
    ((5, 5, 5), [(5, 5, 5)]),
    ((6, 5, 5), [(6, 5, 5)]),
    ((11, 10, 10), [(11, 10, 10), (6, 6, 6)]),
    ((16, 16, 16), [(16, 16, 16), (9, 9, 9)]),
    ((17, 17, 17), [(17, 17, 17), (9, 9, 9)]),
    ((18, 18, 18), [(18, 18, 18), (10, 10, 10)]),
    ((32, 16, 16), [(32, 16, 16), (17, 9, 9), (9, 5, 5)]),
    ((33, 16, 16), [(33, 16, 16), (17, 9, 9), (9, 5, 5)]),
    ((21, 20, 19), [(21, 20, 19), (11, 11, 10), (6, 6, 6)]),
    ((5, 5, 41), [(5, 5, 41), (3, 3, 21)]),
    ((4, 63, 5), [(4, 63, 5), (3, 32, 3)]),
    ((64, 6, 5), [(64, 6, 5), (33, 4, 3)]),
    ((3, 3, 120), [(3, 3, 120), (2, 2, 61)]),
    ((120, 3, 3), [(120, 3, 3), (61, 2, 2)]),
]
EDGE_LEVELS = dict(EDGE_SHAPES)
# "liq" on the two 3-wide shapes has one fluid column, no empty cell and no pressure fixing: the system is singular and the
# reference itself does not converge on it.  Every other shape x kind is a case: 15 x 4 - 2 = 58 in all.
EDGE_CASES = [(kind, dims) for dims, _ in EDGE_SHAPES for kind in KINDS if not (kind == "liq" and min(dims) == 3 and max(dims) == 120)]
FRACTIONS_EDGE_DIMS = (18, 18, 18)


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


def edge_stage_systems(kind, dims):
    """the stage systems of an edge case -> [(tag, flags, A, rhs)]: "lap", the MakeLaplaceMatrix system of stage_inputs, and for
    "gf" also "coef", the coefficient system solvePressure really builds (the ghost-fluid diagonal applied; non-integer entries,
    so the order in which the reference sums its sorted level-1 paths shows).  Built by the plain-C checker library; the
    recorder asserts that the reference builds the same bits."""
    sx, sy, sz = dims
    flags, A, rhs = stage_inputs(kind, dims)
    out = [("lap", flags, A, rhs)]
    if KINDS[kind][2]:
        phi = inputs(kind, dims)[2]
        impl = util.Impl("oracle")
        a0 = impl.dev(A[0].copy())      # on the host impl.dev shares the array's memory
        impl.call("mf_apply_ghost_fluid_diagonal", sx, sy, sz, a0, impl.dev(flags), impl.dev(phi), ctypes.c_float(1e-4), None)
        out.append(("coef", flags, [impl.host(a0).copy(), A[1], A[2], A[3]], rhs))
    return out


def fractions_edge_system():
    """the fill-fraction coefficient system at FRACTIONS_EDGE_DIMS -> flags, fractions, A, rhs"""
    dims, flags, vel, fr = fractions_inputs_model(FRACTIONS_EDGE_DIMS)
    A = cases.run_laplace_impl(util.Impl("oracle"), dims, flags, fr)
    return flags, fr, A, cases.cg_rhs(dims, flags, 7)


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


def fractions_inputs_model(dims=FRACTIONS_DIMS):
    """the obstacle loop's start by the numpy model: updateFractions(boundaryWidth=0), setObstacleFlags(fractions, boundaryWidth=1),
    fillGrid -> dims, flags, vel, fractions"""
    import obstacle_model as OM
    f, phi, vel = OM.loop_inputs(dims)
    fr = OM.update_fractions(f, phi, 0)
    f = OM.set_obstacle_flags(f, phi, fractions=fr, boundaryWidth=1)
    keep = (f & (OM.OBSTACLE | OM.INFLOW | OM.OUTFLOW | OM.OPEN)) != 0
    f = np.where(keep, f, (f & ~(OM.EMPTY | OM.FLUID)) | OM.FLUID).astype(np.int32)
    return dims, f, vel, fr


# ---- the level-by-level fixture (tests/golden/multigrid_levels.npz) --------------------------------------------------------------
FRACTIONS_EDGE_TAG = "fractions_%dx%dx%d__coef" % FRACTIONS_EDGE_DIMS


def edge_stage_tags():
    """every recorded stage system: <kind>_<size>__lap for the 58 edge cases, __coef in addition for "gf", and the fractions case"""
    tags = []
    for kind, dims in EDGE_CASES:
        tags.append(case_name(kind, dims) + "__lap")
        if KINDS[kind][2]:
            tags.append(case_name(kind, dims) + "__coef")
    return tags + [FRACTIONS_EDGE_TAG]


def edge_stage_system(tag):
    """tag -> dims, A (four planes), rhs"""
    if tag == FRACTIONS_EDGE_TAG:
        flags, fr, A, rhs = fractions_edge_system()
        return FRACTIONS_EDGE_DIMS, A, rhs
    name, sysname = tag.split("__")
    kind, size = name.split("_")
    dims = tuple(int(s) for s in size.split("x"))
    for s, flags, A, rhs in edge_stage_systems(kind, dims):
        if s == sysname:
            return dims, A, rhs
    raise KeyError(tag)


def sha256(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def recorded_mismatch(g, key, got):
    """None if `got` has the bits of the recorded array `key` (stored as itself, or as key__sha when it has more than 4096
    elements), else a description of the difference"""
    got = np.ascontiguousarray(got)
    if key in g.files:
        want = g[key]
        if want.shape != got.shape or want.dtype != got.dtype:
            return "%s: %s %s recorded, %s %s given" % (key, want.dtype, want.shape, got.dtype, got.shape)
        if want.tobytes() == got.tobytes():
            return None
        bad = np.nonzero(want.reshape(-1).view(np.uint8 if want.dtype == np.uint8 else np.int32) !=
                         got.reshape(-1).view(np.uint8 if got.dtype == np.uint8 else np.int32))[0]
        i = int(bad[0])
        return "%s: %d of %d values differ from the recording; first at %d: %r, recorded %r" % (
            key, len(bad), want.size, i, got.reshape(-1)[i], want.reshape(-1)[i])
    if sha256(got) == bytes(g[key + "__sha"]).hex():
        return None
    return "%s: the SHA-256 of the %d values differs from the recorded digest" % (key, got.size)


def model_hierarchy(g, tag, dims, A):
    """the numpy model's hierarchy of a recorded stage system (the recorded level-1 operator goes in where the file holds one)"""
    import mg_model
    patch = (g[tag + "__A1fix_idx"], g[tag + "__A1fix_val"]) if tag + "__A1fix_idx" in g.files else None
    return mg_model.setup(dims, A, A1_patch=patch)
