"""CPU: the public face of moving obstacles and obstacle coupling without a GPU -- every new name with its signature, the row of the
open extension table with its header under include/open/, the kernels' file in the Makefile, both refusals (before anything is touched
and before any scratch grid is taken), the shapes' setters in fp32, MovingObstacle's ID counter, and that extrapolateMACSimple without
phiObs still takes the old entry."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest

import movingobs_model as M

WHAT = "moving obstacles and obstacle coupling"
f32 = np.float32
GOLDEN = np.load(M.GOLDEN)

PLUGINS = {
    "set_wall_bcs2": "(flags, vel, obvel)",
    "resetPhiInObs": "(flags, sdf)",
    "extrapolateMACSimple": "(flags, vel, distance=4, phiObs=None, intoObs=False)",
    "resetMovingObstacleState": "()",
}
METHODS = {
    ("MovingObstacle", "__init__"): "(self, parent, emptyType=4, name='', **kw)",
    ("MovingObstacle", "add"): "(self, shape)",
    ("MovingObstacle", "moveLinear"): "(self, t, t0, t1, p0, p1, flags, vel, smooth=True)",
    ("MovingObstacle", "projectOutside"): "(self, flags, flip)",
    ("BasicParticleSystem", "projectOutside"): "(self, gradient)",
    ("Box", "setCenter"): "(self, center)",
    ("Sphere", "setCenter"): "(self, center)",
    ("Cylinder", "setCenter"): "(self, center)",
    ("Cylinder", "setRadius"): "(self, r)",
    ("Cylinder", "setZ"): "(self, z)",
    ("MACGrid", "set_bound_MAC2"): "(self, value, boundaryWidth)",
    ("MACGrid", "setBoundMAC"): "(self, value, boundaryWidth, normalOnly=False)",
    ("FlagGrid", "mark_surface"): "(self)",
    ("FlagGrid", "clear_obstacle"): "(self, include_boundary=False)",
    ("RealGrid", "clamp_norm"): "(self, val)",
    ("LevelsetGrid", "clamp_norm"): "(self, val)",
    ("VecGrid", "clamp_norm"): "(self, val)",
    ("MACGrid", "clamp_norm"): "(self, val)",
}
ENTRIES = {"mf_movingobs_abi_version", "mf_movingobs_set_wall_bcs2", "mf_movingobs_set_bound_mac", "mf_movingobs_mark_surface",
           "mf_movingobs_clear_obstacle", "mf_movingobs_clamp_norm", "mf_movingobs_reset_phi_in_obs", "mf_movingobs_extrapolate_mac_simple",
           "mf_movingobs_move", "mf_movingobs_obstacle_sign", "mf_movingobs_gradient", "mf_movingobs_project_scratch",
           "mf_movingobs_project_count", "mf_movingobs_project_apply"}


def test_names_and_signatures():
    import manta as m
    for name, sig in PLUGINS.items():
        assert str(inspect.signature(getattr(m, name))) == sig, name
    for (cls, name), sig in METHODS.items():
        assert str(inspect.signature(getattr(getattr(m, cls), name))) == sig, (cls, name)
    assert m.FlagEmpty == 4 and not hasattr(m.IntGrid, "mark_surface") and not hasattr(m.IntGrid, "clamp_norm")
    # what other files pin as absent stays absent
    for name in ("obstacleLevelset", "obstacleGradient", "reinitMarching", "particleSurfaceTurbulence", "VortexSheetMesh", "VICintegration",
                 "smoothVorticity", "vorticitySource", "texcoordInflow", "meshSmokeInflow", "resampeOverfullCells", "dissolveSmoke",
                 "quantizeGrid", "resampleVec3ToMac", "fillHoles", "Slope", "NullShape"):
        assert not hasattr(m, name), name
    assert not hasattr(m.FlagGrid, "fillHoles")


def test_row_header_and_version_macro():
    from mantaflow_amd import _lib
    e = _lib.extension("movingobs")
    assert e in _lib.OPEN_EXTENSIONS and (e.what, e.verb) == (WHAT, "do")
    inc = os.path.dirname(_lib.HEADER)
    assert e.header == os.path.join(inc, "open", "manta_hip_movingobs.h") == _lib.MOVINGOBS_HEADER and os.path.exists(e.header)
    assert {x.header for x in _lib.OPEN_EXTENSIONS} == set(glob.glob(os.path.join(inc, "open", "manta_hip_*.h")))
    assert (e.version_fn, e.version_macro) == ("mf_movingobs_abi_version", "MF_MOVINGOBS_ABI_VERSION")
    text = open(e.header).read()
    assert re.search(r"^#define\s+MF_MOVINGOBS_ABI_VERSION\s+1\s*$", text, flags=re.M)
    assert re.search(r"^#define\s+MF_MOVINGOBS_MAX_SHAPES\s+16\s*$", text, flags=re.M)        # the stated cap on the shapes of one move
    restype, argtypes, _ = _lib.parse_header(e.header)[e.version_fn]
    assert restype is ctypes.c_int and argtypes == []


def test_entry_names_are_disjoint_from_every_other_header():
    from mantaflow_amd import _lib
    seen = {n: "manta_hip.h" for n in _lib.parse_header()}
    for e in _lib.all_extensions():
        if e.name != "movingobs":
            for n in _lib.parse_header(e.header):
                seen[n] = os.path.basename(e.header)
    mine = _lib.parse_header(_lib.MOVINGOBS_HEADER)
    assert set(mine) == ENTRIES and all(n.startswith("mf_movingobs_") for n in mine)
    for n in mine:
        assert n not in seen, "%s is declared by %s as well" % (n, seen.get(n))
    for n, (_, _, argnames) in mine.items():
        if n not in ("mf_movingobs_abi_version", "mf_movingobs_project_scratch"):
            assert argnames[-1] == "stream", n


def test_the_kernels_are_built_into_the_library():
    from mantaflow_amd import _lib
    csrc = os.path.join(os.path.dirname(_lib.DEFAULT_LIB))
    make = open(os.path.join(csrc, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", make, flags=re.M).group(1).split()
    assert "movingobs.hip" in srcs and os.path.exists(os.path.join(csrc, "movingobs.hip"))
    text = open(os.path.join(csrc, "movingobs.hip")).read()
    for n in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
    assert "hipcub" not in text and "rocprim" not in text and "-ffp-contract=off" in make
    # one definition each: the passes of extrapolateMACSimple and Shape::isInside live in headers that both users include
    glue, surface = open(os.path.join(csrc, "glue.hip")).read(), open(os.path.join(csrc, "surface.hip")).read()
    passes, inside = open(os.path.join(csrc, "extrap_passes.h")).read(), open(os.path.join(csrc, "shape_inside.h")).read()
    for k in ("k_extrap_mark", "k_extrap_simple", "k_extrap_simple4", "k_extrap_into_bnd"):
        assert re.search(r"void __launch_bounds__\(BLOCK\)\s*%s\(" % k, passes) and not re.search(r"\b%s\(Dim" % k, glue + text), k
    assert '#include "extrap_passes.h"' in glue and '#include "extrap_passes.h"' in text
    assert "int shape_inside(" in inside and "int shape_inside(" not in surface + text
    assert '#include "shape_inside.h"' in surface and '#include "shape_inside.h"' in text


def test_cpu_backend_lacks_the_extension(oracle_backend):
    import manta as m
    from mantaflow_amd import _lib
    assert _lib.get().movingobs is False
    assert m.Solver(name="o", gridSize=m.vec3(8, 7, 6), dim=3).lib.movingobs is False


# ---- a small scene on the CPU backend ---------------------------------------------------------------------------------------------
DIMS = (7, 5, 4)


class Stage(object):
    def __init__(self, m):
        sx, sy, sz = DIMS
        s = self.s = m.Solver(name="o", gridSize=m.vec3(*DIMS), dim=3)
        self.real, self.phi = s.create(m.RealGrid), s.create(m.LevelsetGrid)
        self.mac, self.mac2, self.vec, self.flags = s.create(m.MACGrid), s.create(m.MACGrid), s.create(m.VecGrid), s.create(m.FlagGrid)
        self.grids = dict(real=self.real, phi=self.phi, mac=self.mac, mac2=self.mac2, vec=self.vec, flags=self.flags)
        rng = np.random.RandomState(5)
        for g in (self.real, self.phi):
            g.from_numpy((rng.rand(sz, sy, sx) - 0.5).astype(f32))
        for g in (self.mac, self.mac2, self.vec):
            g.from_numpy(rng.rand(sz, sy, sx, 3).astype(f32))
        self.flags.from_numpy(rng.randint(1, 4, (sz, sy, sx)).astype(np.int32) | (1 << 10))
        self.parts = s.create(m.BasicParticleSystem)
        self.parts.set_positions(rng.rand(9, 3).astype(f32) * 4, rng.randint(0, 2, 9).astype(np.int32))
        m.resetMovingObstacleState()
        self.box = m.Box(parent=s, p0=m.vec3(1, 1, 1), p1=m.vec3(3, 3, 3))
        self.mo = m.MovingObstacle(s)
        self.mo.add(self.box)

    def snapshot(self):
        from mantaflow_amd import core
        snap = {k: g.to_numpy().copy() for k, g in self.grids.items()}
        snap["pos"], snap["pflag"] = self.parts.get_positions().copy(), self.parts.get_flags().copy()
        snap["box"] = (tuple(self.box.p0), tuple(self.box.p1))
        snap["live"] = self.s._live
        snap["pooled"] = {k: len(v) for k, v in self.s._pool.items()}
        snap["ids"] = core._movingobs().id_count
        snap["drawn"] = core._movingobs().rs.bg.state["state"]["pos"]
        return snap

    def unchanged(self, snap):
        now = self.snapshot()
        for k in snap:
            assert np.array_equal(now[k], snap[k]) if isinstance(snap[k], np.ndarray) else now[k] == snap[k], k


def calls(m, S):
    """name -> calls with good arguments and with bad ones: the refusals come before every check"""
    v0 = m.vec3(0, 0, 0)
    return {
        "set_wall_bcs2": (lambda: m.set_wall_bcs2(S.flags, S.mac, S.mac2), lambda: m.set_wall_bcs2(S.flags, S.mac, obvel=S.real)),
        "resetPhiInObs": (lambda: m.resetPhiInObs(S.flags, S.phi), lambda: m.resetPhiInObs(flags=S.mac, sdf=S.phi)),
        "extrapolateMACSimple": (lambda: m.extrapolateMACSimple(S.flags, S.mac, 2, S.phi, True), lambda: m.extrapolateMACSimple(S.flags, S.mac, phiObs=S.real)),
        "MACGrid::set_bound_MAC2": (lambda: S.mac.set_bound_MAC2(v0, 1), lambda: S.mac.set_bound_MAC2("x", 1)),
        "MACGrid::setBoundMAC": (lambda: S.mac.setBoundMAC(v0, 1), lambda: S.mac.setBoundMAC(value=v0, boundaryWidth=0, normalOnly=True)),
        "FlagGrid::mark_surface": (lambda: S.flags.mark_surface(),),
        "FlagGrid::clear_obstacle": (lambda: S.flags.clear_obstacle(), lambda: S.flags.clear_obstacle(include_boundary=True)),
        "Grid::clamp_norm": (lambda: S.real.clamp_norm(0.1), lambda: S.phi.clamp_norm(val=0.0)),
        "VecGrid::clamp_norm": (lambda: S.vec.clamp_norm(0.1),),
        "MACGrid::clamp_norm": (lambda: S.mac.clamp_norm(0.1),),
        "MovingObstacle::moveLinear": (lambda: S.mo.moveLinear(0.5, 0.0, 1.0, m.vec3(2, 2, 2), m.vec3(4, 3, 2), S.flags, S.mac),
                                       lambda: S.mo.moveLinear(0.5, 0.0, 1.0, m.vec3(2, 2, 2), m.vec3(4, 3, 2), S.mac, S.flags, smooth=False),
                                       lambda: S.mo.moveLinear(5.0, 0.0, 1.0, m.vec3(2, 2, 2), m.vec3(4, 3, 2), S.flags, S.mac)),
        "MovingObstacle::projectOutside": (lambda: S.mo.projectOutside(S.flags, S.parts), lambda: S.mo.projectOutside(S.flags, None)),
        "BasicParticleSystem::projectOutside": (lambda: S.parts.projectOutside(S.vec), lambda: S.parts.projectOutside(S.real)),
    }


@pytest.mark.parametrize("name", ["set_wall_bcs2", "resetPhiInObs", "extrapolateMACSimple", "MACGrid::set_bound_MAC2", "MACGrid::setBoundMAC",
                                  "FlagGrid::mark_surface", "FlagGrid::clear_obstacle", "Grid::clamp_norm", "VecGrid::clamp_norm", "MACGrid::clamp_norm",
                                  "MovingObstacle::moveLinear", "MovingObstacle::projectOutside", "BasicParticleSystem::projectOutside"])
def test_refused_on_the_cpu_backend_and_on_a_z_slab_solver(oracle_backend, name):
    import manta as m
    S = Stage(m)
    snap = S.snapshot()
    assert set(calls(m, S)) >= {name}
    for call in calls(m, S)[name]:
        with pytest.raises(RuntimeError) as err:
            call()
        assert str(err.value) == "%s: the 'oracle' backend does not implement %s (manta_hip_movingobs.h)" % (name, WHAT)
        S.unchanged(snap)
        S.s._slab_window = (4, 40)      # what slab.SlabDomain gives the solver of a z-slab: (z offset, global sz)
        try:
            with pytest.raises(RuntimeError) as err:
                call()
            assert str(err.value) == "%s: %s do not run on a z-slab solver" % (name, WHAT)      # the z-slab check comes first
        finally:
            S.s._slab_window = (0, 0)
        S.unchanged(snap)
    m.resetMovingObstacleState()


def test_turbulence_particles_keep_their_own_refusal(oracle_backend):
    import manta as m
    assert m.TurbulenceParticleSystem.projectOutside is not m.BasicParticleSystem.projectOutside
    assert "not implemented" in inspect.getsource(m.TurbulenceParticleSystem.projectOutside)


def test_without_phi_obs_the_old_entry_runs(oracle_backend):
    """on the CPU backend, which has mf_extrapolate_mac_simple and lacks this extension: None and 0 both mean "no phiObs" """
    import manta as m
    S = Stage(m)
    f, v, _, _ = M.extrap_inputs("a")
    s = m.Solver(name="p", gridSize=m.vec3(*M.DIMS["a"]), dim=3)
    flags, vel = s.create(m.FlagGrid), s.create(m.MACGrid)
    flags.from_numpy(f)
    for none in (None, 0):
        vel.from_numpy(v)
        m.extrapolateMACSimple(flags, vel, M.EXTRAP_DISTANCE, none, False)
        assert M.same(vel.to_numpy(), GOLDEN["extrap/a/plain"])
    vel.from_numpy(v)
    m.extrapolateMACSimple(flags, vel, distance=M.EXTRAP_DISTANCE)
    assert M.same(vel.to_numpy(), GOLDEN["extrap/a/plain"])
    del S


# ---- host code that runs on every backend ------------------------------------------------------------------------------------------
def shape_state(sh, kind):
    o = np.zeros(8, f32)
    if kind == 0:
        o[0:3], o[3:6] = list(sh.p0), list(sh.p1)
    else:
        o[0:3], o[3] = list(sh.center), sh.radius
        if kind == 2:
            o[4:7] = [f32(sh.zlen) * f32(x) for x in sh.zdir]
    return o


def test_shape_setters_are_fp32_and_invalidate_the_cached_sdf(oracle_backend):
    import manta as m
    s = m.Solver(name="o", gridSize=m.vec3(8, 8, 8), dim=3)
    for q, (kind, a, centre, doCyl, r, z) in enumerate(M.SETTER_CASES):
        if kind == 0:
            sh = m.Box(parent=s, p0=m.vec3(*a[0:3]), p1=m.vec3(*a[3:6]))
        elif kind == 1:
            sh = m.Sphere(parent=s, center=m.vec3(*a[0:3]), radius=a[3], scale=m.vec3(*a[4:7]))
        else:
            sh = m.Cylinder(parent=s, center=m.vec3(*a[0:3]), radius=a[3], z=m.vec3(*a[4:7]))
        before = sh.computeLevelset().to_numpy().copy()
        sh.setCenter(m.vec3(*centre))
        if kind == 2 and doCyl:
            sh.setRadius(r)
            sh.setZ(m.vec3(*z))
        assert M.same(shape_state(sh, kind), GOLDEN["setters/%d/state" % q]), q
        assert M.same(np.array([f32(x) for x in sh.getCenter()], f32), GOLDEN["setters/%d/centre" % q]), q
        after = sh.computeLevelset().to_numpy()
        assert not np.array_equal(before, after, equal_nan=True), q            # the cache key saw the new parameters
    base = m.Shape(s)
    base.setCenter(m.vec3(1, 2, 3))
    assert tuple(base.getCenter()) == (0, 0, 0)
    with pytest.raises(RuntimeError, match="can't convert argument to Vec3"):
        sh.setCenter("here")


def test_id_allocation(oracle_backend):
    import manta as m
    s = m.Solver(name="o", gridSize=m.vec3(8, 8, 8), dim=3)
    m.resetMovingObstacleState()
    want = [int(x) for x in GOLDEN["ids/ids"][:5]]
    assert want == [1 << 10, 1 << 11, 1 << 12, 1 << 13, 1 << 14]
    obs = [m.MovingObstacle(s), m.MovingObstacle(parent=s, emptyType=m.FlagEmpty | m.FlagStick), m.MovingObstacle(s), m.MovingObstacle(s), m.MovingObstacle(s)]
    assert [o.mID for o in obs] == want and obs[1].mEmptyType == 68 and obs[0].mEmptyType == m.FlagEmpty
    message = bytes(GOLDEN["ids/message"]).decode()
    for k in (6, 7):
        with pytest.raises(RuntimeError) as err:
            m.MovingObstacle(s)
        assert str(err.value) == message
    from mantaflow_amd import core
    assert core._movingobs().id_count == int(GOLDEN["ids/after"][0]) == 17          # the counter moved before each raise
    m.resetMovingObstacleState()
    assert core._movingobs().id_count == 10 and m.MovingObstacle(s).mID == 1 << 10
    with pytest.raises(RuntimeError, match="no parent given"):
        m.MovingObstacle(None)
    with pytest.raises(RuntimeError, match=r"can't convert argument to Shape\*"):
        m.MovingObstacle(s).add(s.create(m.RealGrid))
    m.resetMovingObstacleState()


def test_the_projection_stream_is_the_reference_s_and_resets(oracle_backend):
    import manta as m
    from mantaflow_amd import core
    m.resetMovingObstacleState()
    a = core._movingobs().rs.reals(5)
    ref = M.Stream()
    assert M.same(a, np.array([ref.real() for _ in range(5)], f32))
    b = core._movingobs().rs.reals(5)
    assert not M.same(a, b)
    m.resetMovingObstacleState()
    assert M.same(core._movingobs().rs.reals(5), a)
    m.resetMovingObstacleState()
