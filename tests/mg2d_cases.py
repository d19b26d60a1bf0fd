"""Inputs shared by the tests of the 2-D multigrid hierarchy (test_mg2d_model.py, test_mg2d_api.py, test_gpu_mg2d.py) and by its
recorder tools/record_mg2d.py.  Inputs are regenerated from the seeded generators of tests/util.py and tests/mg_cases.py (which are
dimension-free), never stored; dims are (sx, sy, 1).

The shapes are the smallest at which each piece of the hierarchy can go wrong; the level sizes GridMg must give them (coarsening by
(s + 2) / 2 stops when both axes are <= 5 or the level has <= 1000 vertices) are pinned here and checked against the size rule."""
import os

import numpy as np

import cases
import mg_cases
import util
from mg_cases import KINDS, PcMGDynamic, PcMGStatic, PcMIC, case_name, recorded_mismatch, sha256  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mg2d.npz")      # recorded by tools/record_mg2d.py
TAIL_VERTS = 8192      # mg2d.hip: levels of at most this many vertices run in the single-workgroup kernel

SHAPES = [
    # one level: the coarsest-level CG alone; the last with exactly 1000 vertices
    ((5, 5, 1), [(5, 5, 1)]),
    ((30, 30, 1), [(30, 30, 1)]),
    ((40, 25, 1), [(40, 25, 1)]),
    # the first shape with a coarse level
    ((32, 32, 1), [(32, 32, 1), (17, 17, 1)]),
    # mixed parities at the restriction / interpolation edges
    ((33, 31, 1), [(33, 31, 1), (17, 16, 1)]),
    # a coarsest level of exactly 1000 vertices
    ((78, 48, 1), [(78, 48, 1), (40, 25, 1)]),
    # thin levels, one interior column (none at all in the 2-wide one: every vertex is inactive)
    ((3, 400, 1), [(3, 400, 1), (2, 201, 1)]),
    ((400, 3, 1), [(400, 3, 1), (201, 2, 1)]),
    ((2, 600, 1), [(2, 600, 1), (2, 301, 1)]),
    # level 0 on either side of the 8192-vertex hand-over (8190 / 8281 vertices)
    ((90, 91, 1), [(90, 91, 1), (46, 46, 1), (24, 24, 1)]),
    ((91, 91, 1), [(91, 91, 1), (46, 46, 1), (24, 24, 1)]),
    # three levels with random obstacles
    ((129, 97, 1), [(129, 97, 1), (65, 49, 1), (33, 25, 1)]),
    # level 1 above 8192 vertices: the only shape where the four-colour kernels and the generic operator run grid-wide
    ((257, 130, 1), [(257, 130, 1), (129, 66, 1), (65, 34, 1), (33, 18, 1)]),
]
LEVELS = dict(SHAPES)

# Exclusions, by name: a case on which the reference itself does not converge in fewer than 100 iterations is not a case.  On the
# two 3-wide shapes the fluid is a single column (row) of cells, and the obstacle blobs of "obs" / "liq" / "gf" cut it into
# closed segments.  A segment without an empty cell and without a fixed pressure makes the system singular (zeroPressureFixing
# fixes one cell of the whole grid, and the "liq" / "gf" empty band touches only the top segment of 3x400 and nothing of 400x3,
# whose top row is wall).  The reference runs into its 100 iterations on five of them and stops with "The CG solver diverged" on
# the sixth.  "box" has one connected column and converges; it stays a case on both shapes.
# The recorder (tools/record_mg2d.py) asserts that every case NOT listed converged in fewer than 100 iterations with both
# preconditioners, and that every case listed did not.  No other case is left out, on the CPU or on the GPU.
_SEGMENTS = "a single fluid column cut into closed segments by the obstacle blobs: singular, the reference "
EXCLUDED = {
    "obs_3x400x1": _SEGMENTS + "runs into its 100 iterations",
    "liq_3x400x1": _SEGMENTS + "stops with 'The CG solver diverged'",
    "gf_3x400x1": _SEGMENTS + "runs into its 100 iterations",
    "obs_400x3x1": _SEGMENTS + "runs into its 100 iterations",
    "liq_400x3x1": _SEGMENTS + "runs into its 100 iterations",
    "gf_400x3x1": _SEGMENTS + "runs into its 100 iterations",
}
CASES = [(kind, dims) for dims, _ in SHAPES for kind in KINDS if case_name(kind, dims) not in EXCLUDED]
FRACTIONS_DIMS = (40, 32, 1)
FRACTIONS_LEVELS = [(40, 32, 1), (21, 17, 1)]
FRACTIONS_NAME = "fractions_%dx%dx%d" % FRACTIONS_DIMS
FRACTIONS_KW = dict(cgAccuracy=1e-3)


def inputs(kind, dims, vel_seed=1):
    """flags, velocity (after setWallBcs), phi or None, solvePressure arguments"""
    return mg_cases.inputs(kind, dims, vel_seed)


def fractions_inputs():
    """the obstacle loop's start by the numpy model at FRACTIONS_DIMS -> flags, vel, fractions"""
    _, f, vel, fr = mg_cases.fractions_inputs_model(FRACTIONS_DIMS)
    return f, vel, fr


def planes3(A):
    """the three planes a 2-D system has, of the four the generators make (Ak is all zero in 2-D)"""
    assert not np.asarray(A[3]).any()
    return [np.ascontiguousarray(a, np.float32) for a in A[:3]]


def stage_systems(kind, dims):
    """the stage systems of a case -> [(tag, A (three planes), rhs)]: "lap", MakeLaplaceMatrix of the kind's flags, and for "gf"
    also "coef", the coefficient system solvePressure really builds (the ghost-fluid diagonal applied)"""
    return [(sysname, planes3(A), rhs) for sysname, flags, A, rhs in mg_cases.edge_stage_systems(kind, dims)]


def fractions_system():
    """the fill-fraction coefficient system at FRACTIONS_DIMS -> A (three planes), rhs"""
    flags, vel, fr = fractions_inputs()
    A = cases.run_laplace_impl(util.Impl("oracle"), FRACTIONS_DIMS, flags, fr)
    return planes3(A), cases.cg_rhs(FRACTIONS_DIMS, flags, 7)


def stage_tags():
    """every recorded stage system: <kind>_<size>__lap for every case, __coef in addition for "gf", and the fractions case"""
    tags = []
    for kind, dims in CASES:
        tags.append(case_name(kind, dims) + "__lap")
        if KINDS[kind][2]:
            tags.append(case_name(kind, dims) + "__coef")
    return tags + [FRACTIONS_NAME + "__coef"]


def stage_system_dims(tag):
    name = tag.split("__")[0]
    return FRACTIONS_DIMS if name == FRACTIONS_NAME else tuple(int(v) for v in name.split("_")[1].split("x"))


def stage_system(tag):
    """tag -> dims, A (three planes), rhs"""
    name, sysname = tag.split("__")
    if name == FRACTIONS_NAME:
        return (FRACTIONS_DIMS,) + fractions_system()
    kind, size = name.split("_")
    dims = tuple(int(s) for s in size.split("x"))
    for s, A, rhs in stage_systems(kind, dims):
        if s == sysname:
            return dims, A, rhs
    raise KeyError(tag)


def model_hierarchy(g, tag, dims, A):
    """the numpy model's hierarchy of a recorded stage system (the recorded level-1 operator goes in where the file holds one)"""
    import mg2d_model
    patch = (g[tag + "__A1fix_idx"], g[tag + "__A1fix_val"]) if tag + "__A1fix_idx" in g.files else None
    return mg2d_model.setup(dims, A, A1_patch=patch)


def expected_tail_first(sizes, tail_verts=TAIL_VERTS):
    first = len(sizes) - 1
    while first > 0 and sizes[first - 1][0] * sizes[first - 1][1] <= tail_verts:
        first -= 1
    return first


# ---- Static semantics: two solves with different flags on one solver ------------------------------------------------------------------
STATIC_DIMS = (90, 91, 1)
STATIC_KW = dict(cgAccuracy=1e-3, zeroPressureFixing=True)


def static_pair():
    """[(flags, vel)] x 2: (a) the "obs" inputs, (b) an obstacle blob added and another velocity -- under PcMGStatic the hierarchy of
    (a) then preconditions a matrix it was not built from"""
    sx, sy, _ = STATIC_DIMS
    fa, va, _, _ = inputs("obs", STATIC_DIMS)
    fb = fa.copy()
    yy, xx = np.ogrid[:sy, :sx]
    blob = ((xx - 60) ** 2 + (yy - 30) ** 2 <= 9)[None]
    fb[blob & (fb == util.FLUID)] = util.OBS
    assert (fb != fa).sum() > 10
    vb = mg_cases.wall_bcs(STATIC_DIMS, fb, util.smooth_vel(sx, sy, 1, 3))
    return [(fa, va), (fb, vb)]


# ---- the three recorded loops -------------------------------------------------------------------------------------------------------
# tests/mg2d_loops.py states them for the package, tools/mg2d_record.cpp the same plugin calls against the reference's headers.
PLUME = dict(res=64, steps=4)
GUIDING = dict(res0=40, scale=1, steps=2)
# (the dam's fluid cells change for the first time in step 3; a Static hierarchy that is older than the flags makes the reference's
# own solve run into its 100 iterations or diverge, so the release comes before that step)
FLIP = dict(res=48, steps=4, release_after=3)
