"""GPU: moving obstacles and obstacle coupling (include/open/manta_hip_movingobs.h) on the device against the reference's recorded
outputs (tests/golden/movingobs.npz), bit for bit, on the three grids of tests/movingobs_model.py: (6, 5, 4), (13, 9, 8) -- more than one
workgroup of 256 cells -- and the 2-D (8, 7, 1).

MovingObstacle.moveLinear is compared with the recording as far as the reference library could run (the shapes' new centres, the reset
flags; everything where alpha is outside [0, 1] or the obstacle has no shape) and, for the stamping of the shapes and the velocity
pass, with the numpy model alone: MODEL PARITY, not reference parity (see movingobs_model's docstring).  The same holds for the
end-to-end loop, which drives moveLinear every step."""
import numpy as np
import pytest

import movingobs_model as M

pytestmark = pytest.mark.gpu

GOLDEN = np.load(M.GOLDEN)
f32 = np.float32
GRIDS = sorted(M.DIMS)


def solver(m, g):
    dims = M.DIMS[g]
    return m.Solver(name="s", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)


def grid_from(s, cls, a):
    g = s.create(cls)
    g.from_numpy(a)
    return g


def same(tag, got, want):
    assert M.same(got, want), "%s: %d of %d elements differ" % (tag, M.differing(np.asarray(got), np.asarray(want)), np.asarray(want).size)


def particles_from(m, s, pos, flag):
    p = s.create(m.BasicParticleSystem)
    p.set_positions(pos, flag)
    return p


def make_shape(m, s, kind, a):
    if kind == 0:
        return m.Box(parent=s, p0=m.vec3(*a[0:3]), p1=m.vec3(*a[3:6]))
    if kind == 1:
        return m.Sphere(parent=s, center=m.vec3(*a[0:3]), radius=a[3], scale=m.vec3(*a[4:7]))
    return m.Cylinder(parent=s, center=m.vec3(*a[0:3]), radius=a[3], z=m.vec3(*a[4:7]))


def shape_state(sh, kind):
    """the 8 floats tools/movingobs_record.cpp reports for a shape"""
    o = np.zeros(8, f32)
    if kind == 0:
        o[0:3], o[3:6] = list(sh.p0), list(sh.p1)
    else:
        o[0:3], o[3] = list(sh.center), sh.radius
        if kind == 2:
            o[4:7] = [f32(sh.zlen) * f32(x) for x in sh.zdir]
    return o


@pytest.mark.parametrize("g", GRIDS)
def test_set_wall_bcs2(hip_backend, g):
    import manta as m
    s = solver(m, g)
    f, v, o = M.wall2_inputs(g)
    flags, vel, obvel = grid_from(s, m.FlagGrid, f), grid_from(s, m.MACGrid, v), grid_from(s, m.MACGrid, o)
    m.set_wall_bcs2(flags, vel, obvel=obvel)
    same("vel", vel.to_numpy(), GOLDEN["wall2/" + g])
    same("obvel", obvel.to_numpy(), o)
    same("flags", flags.to_numpy(), f)
    with pytest.raises(RuntimeError, match="must not alias"):
        m.set_wall_bcs2(flags, vel, vel)


@pytest.mark.parametrize("g", GRIDS)
def test_mac_boundary_bands(hip_backend, g):
    import manta as m
    s = solver(m, g)
    val = m.vec3(*[float(x) for x in M.BOUND_VALUE])
    for w in M.BOUND_WIDTHS:
        vel = grid_from(s, m.MACGrid, M.bound_input(g))
        vel.setBoundMAC(val, w)
        same("setBoundMAC %d" % w, vel.to_numpy(), GOLDEN["bound/%s/r0/w%d" % (g, w)])
        vel.from_numpy(M.bound_input(g))
        vel.setBoundMAC(val, w, False)
        same("setBoundMAC %d, normalOnly=False" % w, vel.to_numpy(), GOLDEN["bound/%s/r0/w%d" % (g, w)])
        vel.from_numpy(M.bound_input(g))
        vel.setBoundMAC(value=val, boundaryWidth=w, normalOnly=True)
        same("setBoundMAC %d, normalOnly" % w, vel.to_numpy(), GOLDEN["bound/%s/r1/w%d" % (g, w)])
        vel.from_numpy(M.bound_input(g))
        vel.set_bound_MAC2(val, w)
        same("set_bound_MAC2 %d" % w, vel.to_numpy(), GOLDEN["bound/%s/r2/w%d" % (g, w)])


@pytest.mark.parametrize("g", GRIDS)
def test_mark_surface_and_clear_obstacle(hip_backend, g):
    import manta as m
    s = solver(m, g)
    for kind in M.SURF_KINDS:
        flags = grid_from(s, m.FlagGrid, M.surf_input(g, kind))
        flags.mark_surface()
        same("mark_surface " + kind, flags.to_numpy(), GOLDEN["surf/%s/%s" % (g, kind)])
        flags.mark_surface()                                  # its own output is a fixed point: the stale bits are its own
        same("mark_surface twice " + kind, flags.to_numpy(), GOLDEN["surf/%s/%s" % (g, kind)])
    flags = grid_from(s, m.FlagGrid, M.clear_input(g))
    flags.clear_obstacle()
    same("clear_obstacle()", flags.to_numpy(), GOLDEN["clear/%s/b0" % g])
    for b in (False, True):
        flags.from_numpy(M.clear_input(g))
        flags.clear_obstacle(include_boundary=b)
        same("clear_obstacle(%s)" % b, flags.to_numpy(), GOLDEN["clear/%s/b%d" % (g, int(b))])


@pytest.mark.parametrize("g", GRIDS)
def test_clamp_norm_and_reset_phi(hip_backend, g):
    import manta as m
    s = solver(m, g)
    for kind, cls in (("real", m.RealGrid), ("vec", m.VecGrid), ("mac", m.MACGrid)):
        a = M.cnorm_input(g, "real" if kind == "real" else "vec")
        for q, val in enumerate(M.CNORM_VALS):
            grid = grid_from(s, cls, a)
            grid.clamp_norm(val)
            same("clamp_norm %s %g" % (kind, val), grid.to_numpy(), GOLDEN["cnorm/%s/%s/v%d" % (g, kind, q)])
    ls = grid_from(s, m.LevelsetGrid, M.cnorm_input(g, "real"))
    ls.clamp_norm(val=0.5)
    same("clamp_norm on a LevelsetGrid", ls.to_numpy(), GOLDEN["cnorm/%s/real/v1" % g])
    f, phi = M.reset_inputs(g)
    flags, sdf = grid_from(s, m.FlagGrid, f), grid_from(s, m.LevelsetGrid, phi)
    m.resetPhiInObs(flags, sdf)
    same("resetPhiInObs", sdf.to_numpy(), GOLDEN["reset/" + g])
    same("flags", flags.to_numpy(), f)


@pytest.mark.parametrize("g", GRIDS)
def test_extrapolate_with_phi_obs(hip_backend, g):
    import manta as m
    s = solver(m, g)
    f, v, phi, _ = M.extrap_inputs(g)
    flags, phiObs = grid_from(s, m.FlagGrid, f), grid_from(s, m.LevelsetGrid, phi)
    live = s._live
    for into in (False, True):
        vel = grid_from(s, m.MACGrid, v)
        m.extrapolateMACSimple(flags, vel, M.EXTRAP_DISTANCE, phiObs, into)
        same("intoObs %s" % into, vel.to_numpy(), GOLDEN["extrap/%s/o%d" % (g, int(into))])
        del vel
    vel = grid_from(s, m.MACGrid, v)
    m.extrapolateMACSimple(flags, vel, distance=M.EXTRAP_DISTANCE, phiObs=phiObs)
    same("keywords", vel.to_numpy(), GOLDEN["extrap/%s/o0" % g])
    # without phiObs the old entry runs, and gives what the reference gives without it
    for none in (None, 0):
        vel.from_numpy(v)
        m.extrapolateMACSimple(flags, vel, M.EXTRAP_DISTANCE, none, False)
        same("phiObs %r" % none, vel.to_numpy(), GOLDEN["extrap/%s/plain" % g])
    same("phiObs", phiObs.to_numpy(), phi)
    same("flags", flags.to_numpy(), f)
    del vel
    assert s._live == live                                    # the scratch grids are back in the pool


@pytest.mark.parametrize("case", sorted(M.move_cases()))
def test_move_linear(hip_backend, case):
    import manta as m
    c = M.move_cases()[case]
    s = solver(m, c["grid"])
    s.timestep = M.MOVE_DT
    f0, v0 = M.move_inputs(case)
    flags, vel = grid_from(s, m.FlagGrid, f0), grid_from(s, m.MACGrid, v0)
    m.resetMovingObstacleState()
    for _ in range(c["which"]):
        m.MovingObstacle(s)
    mo = m.MovingObstacle(s, c["emptyType"]) if c["emptyType"] != M.EMPTY else m.MovingObstacle(parent=s)
    assert mo.mID == M.move_id(c["which"])
    shapes = [make_shape(m, s, k, a) for k, a in c["shapes"]]
    for sh in shapes:
        mo.add(sh)
    mo.moveLinear(c["t"], c["t0"], c["t1"], m.vec3(*c["p0"]), m.vec3(*c["p1"]), flags, vel, bool(c["smooth"]))
    got_f, got_v = flags.to_numpy(), vel.to_numpy()
    states = np.array([shape_state(sh, k) for sh, (k, _) in zip(shapes, c["shapes"])], f32).reshape(len(shapes), 8)
    same("the shapes after the call (recorded)", states, GOLDEN["move/%s/states" % case])
    mf, mv, _ = M.move_model(case)
    if "move/%s/flags" % case in GOLDEN.files:
        same("flags (recorded)", got_f, GOLDEN["move/%s/flags" % case])
        same("vel (recorded)", got_v, GOLDEN["move/%s/vel" % case])
    else:
        # recorded: the reset.  Every cell the shapes did not stamp holds the recorded reset flags
        stamped = got_f == (M.OBSTACLE | mo.mID)
        same("reset flags (recorded)", got_f[~stamped], GOLDEN["move/%s/reset_flags" % case][~stamped])
        other = M.move_id((c["which"] + 1) % 5)
        assert ((got_f & other) != 0).any()                   # the other obstacle's cells survive where this one is not
        # model only: the stamping of the shapes and the velocity pass
        same("flags (MODEL)", got_f, mf)
        same("vel (MODEL)", got_v, mv)
        same("flags (the model's stored output)", got_f, GOLDEN["move/%s/model_flags" % case])
        same("vel (the model's stored output)", got_v, GOLDEN["move/%s/model_vel" % case])
    m.resetMovingObstacleState()


def test_move_linear_refuses_more_shapes_than_the_header_allows(hip_backend):
    import manta as m
    s = solver(m, "a")
    flags, vel = s.create(m.FlagGrid), s.create(m.MACGrid)
    m.resetMovingObstacleState()
    mo = m.MovingObstacle(s)
    for _ in range(17):
        mo.add(m.Sphere(parent=s, center=m.vec3(3, 2, 2), radius=1.0))
    with pytest.raises(RuntimeError, match="17 shapes, at most 16"):
        mo.moveLinear(0.5, 0.0, 1.0, m.vec3(2, 2, 2), m.vec3(3, 2, 2), flags, vel)
    assert (flags.to_numpy() == 0).all() and (vel.to_numpy() == 0).all()
    m.resetMovingObstacleState()


def run_projection(m, q):
    what, g, n = M.PROJECT_SEQUENCE[q]
    s = solver(m, g)
    pos, flag = M.particles(g, n, what)
    parts = particles_from(m, s, pos, flag)
    if what == "grad":
        grad = grid_from(s, m.VecGrid, M.gradient_input(g))
        parts.projectOutside(grad)
        same("the gradient", grad.to_numpy(), M.gradient_input(g))
    else:
        flags = grid_from(s, m.FlagGrid, M.obstacle_flags(g))
        m.MovingObstacle(s).projectOutside(flags, parts)
        same("the flags", flags.to_numpy(), M.obstacle_flags(g))
    assert parts.np == n
    same("particle flags", parts.get_flags(), flag)
    return parts.get_positions().reshape(n, 3)


def test_project_outside_in_sequence(hip_backend):
    """0, 1, 65 and 300 particles (deleted ones and ones outside the grid among them), two calls in a row with the same input -- the
    stream goes on --, 2-D, MovingObstacle.projectOutside, and the sequence again from the start after resetMovingObstacleState()"""
    import manta as m
    m.resetMovingObstacleState()
    for q in range(len(M.PROJECT_SEQUENCE)):
        same("step %d %r" % (q, M.PROJECT_SEQUENCE[q]), run_projection(m, q), GOLDEN["proj/%d" % q])
    got = run_projection(m, 2)
    assert not M.same(got, GOLDEN["proj/2"])                 # the stream has moved on
    m.resetMovingObstacleState()
    for q in range(3):
        same("after the reset, step %d" % q, run_projection(m, q), GOLDEN["proj/%d" % q])
    m.resetMovingObstacleState()


def test_flip_loop_with_a_moving_box_model_parity(hip_backend):
    """MODEL PARITY: ten steps of the model's own step list (movingobs_model.LOOP) with a Box moved by moveLinear, whose stamping and
    velocity the reference library cannot run; every other entry in the loop is recorded elsewhere in this file"""
    import manta as m
    L = M.LOOP
    s = solver(m, L["grid"])
    s.timestep = L["dt"]
    f0, v0, phi0, pos0, pflag = M.loop_inputs()
    flags, vel, obvel = grid_from(s, m.FlagGrid, f0), grid_from(s, m.MACGrid, v0), s.create(m.MACGrid)
    phi, phiObs = grid_from(s, m.LevelsetGrid, phi0), s.create(m.LevelsetGrid)
    parts = particles_from(m, s, pos0, pflag)
    m.resetMovingObstacleState()
    box = make_shape(m, s, *L["box"])
    mo = m.MovingObstacle(s)
    mo.add(box)
    for step in range(L["steps"]):
        t = float(f32(step) * f32(L["dt"]))
        mo.moveLinear(t, L["t0"], L["t1"], m.vec3(*L["p0"]), m.vec3(*L["p1"]), flags, obvel, True)
        m.set_wall_bcs2(flags, vel, obvel)
        vel.setBoundMAC(m.vec3(0, 0, 0), 0)
        flags.mark_surface()
        phiObs.from_numpy(np.where((flags.to_numpy() & mo.mID) != 0, f32(-1.0), f32(1.0)).astype(f32))      # the test's own input
        m.extrapolateMACSimple(flags, vel, L["distance"], phiObs, True)
        m.resetPhiInObs(flags, phi)
        vel.clamp_norm(1.5)
        mo.projectOutside(flags, parts)
    want = M.loop_model()
    same("flags", flags.to_numpy(), want["flags"])
    same("obvel", obvel.to_numpy(), want["obvel"])
    same("vel", vel.to_numpy(), want["vel"])
    same("phi", phi.to_numpy(), want["phi"])
    same("positions", parts.get_positions().reshape(-1, 3), want["pos"])
    m.resetMovingObstacleState()
