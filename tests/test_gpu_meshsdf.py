"""GPU: mesh level sets through the package on the HIP backend against the numpy model (tests/meshsdf_model.py) and the recorded
reference (tests/golden/meshsdf.npz; how it was produced: tools/record_meshsdf.py).

Per case: the sources as emitted equal the model's bit for bit, the stats report the model's counts, the pre-flood field differs from the
model's in at most ONE written cell, and there within the bound of DESIGN.md section 17 (a device fp64 exp can round differently from
the host's only next to an fp32 rounding boundary; the count is printed -- on the MI355X it was 0 in every case), and with no such cell
the flooded field equals the model's bit for bit.  Against the reference: differences only in written, unflooded cells and within the
same bound; the flooded set, the written set and every sign are the reference's.  Each case runs twice in a row on one mesh after a
larger call, with the level set, the solver's pool scratch and the mesh's source buffers filled with NaN / garbage in between.

The flood fill alone is also driven through mf_meshsdf_flood on synthetic fields: a U-shaped channel that makes the fill snake across
tile boundaries (more than one productive round, from the stats), seeds in one corner tile only, and random small grids.

The hole that lets the inside flood is the model case sphere_open (a coarse sphere with one triangle removed); a sphere meshed by the
device's own createMesh has cell-sized triangles, so removing one opens no corridor at any usable cutoff: that pair is held to the model
and only the closed one to "the inside stays -cutoff".  The loop of scenes/meshload.py (torus at res 24, 6 smoke steps) runs against a
recorded reference run: flags and CG iterations per step identical, density, velocity and pressure within 1e-5 relative."""
import ctypes
import os

import numpy as np
import pytest

import meshsdf_model as M

pytestmark = pytest.mark.gpu
GOLDEN = np.load(M.GOLDEN)
f32 = np.float32


def _solver(m, dims, name="t"):
    return m.Solver(name=name, gridSize=m.vec3(*dims), dim=3)


def _poison(s, mesh, phi):
    import torch
    for q in range(5):
        s._pool.setdefault("int", []).append(torch.full((s.ncells,), 0x7f7f7f7f - q, dtype=torch.int32, device=s.device))
    mesh._sdf_f.fill_(float("nan"))
    mesh._sdf_i.fill_(0x7f7f7f7f)
    if mesh._sdf_off is not None:
        mesh._sdf_off.fill_(-(1 << 40))
        mesh._sdf_stats.fill_(-7)
    phi.data.fill_(float("nan"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_field(name, R, pre, phi):
    d = np.nonzero(_bits(pre) != _bits(R["pre"]))[0]
    print("%s: %d written cells differ from the model before the flood" % (name, d.size))
    assert d.size <= 1, (name, d[:10], pre[d[:10]], R["pre"][d[:10]])
    assert R["C"]["written"][d].all() and (np.abs(pre[d].astype(np.float64) - R["pre"][d]) <= M.bound(R["C"], R["pre"])[d]).all(), name
    cut = R["P"]["cutoff"]
    if d.size == 0:
        e = _bits(phi) != _bits(R["phi"])
        assert not e.any(), "%s: %d cells differ from the model after the flood, first at %s" % (name, int(e.sum()), np.argwhere(e)[0])
    assert np.array_equal(phi == cut, R["phi"] == cut) and np.array_equal(phi < 0, R["phi"] < 0), name
    if (name + "/sha") in GOLDEN.files:
        ref = M.reference_phi(GOLDEN, name)
        e = np.nonzero(_bits(phi) != _bits(ref))[0]
        flooded = _bits(R["phi"]) != _bits(R["pre"])
        assert R["C"]["written"][e].all() and not flooded[e].any(), name
        assert (np.abs(phi[e].astype(np.float64) - ref[e]) <= M.bound(R["C"], ref)[e]).all(), name
        assert np.array_equal(phi == cut, ref == cut) and np.array_equal(phi < 0, ref < 0), name


def _run_case(m, name, c=None, R=None):
    c, R = c or M.case(name), R or M.model(name)
    sm = _solver(m, c["mesh_gs"], "mesh")
    sg = sm if c["mesh_gs"] == c["dims"] else _solver(m, c["dims"], "grid")
    mesh, phi = sm.create(m.Mesh), sg.create(m.LevelsetGrid)
    # a larger previous call
    nt = c["tris"].shape[0]
    p, t = M.random_tris(max(2 * nt, R["counters"]["sources"]) + 70, c["mesh_gs"], 3, size=2.5)
    mesh.set_numpy(p, None, None, t, None)
    mesh.computeLevelset(phi, 2.)
    assert m.lastMeshSdfStats()["sources"] > R["counters"]["sources"]
    cap = mesh._sdf_cap
    mesh.set_numpy(c["pos"], None, None, c["tris"], None)
    live = sg._live
    for rep in range(2):
        _poison(sg, mesh, phi)
        mesh._mesh_sdf(sm.lib, "test", phi, c["sigma"], c["cutoff"], flood=False)
        pre = phi.to_numpy().reshape(-1)
        st = m.lastMeshSdfStats()
        assert (st["sources"], st["binned"], st["rounds"]) == (R["counters"]["sources"], R["counters"]["binned"], 0), (name, st)
        n = st["sources"]
        if n:
            sg.sync()
            got = mesh._sdf_f.view(12, -1)[:6, :n].cpu().numpy()
            assert np.array_equal(_bits(got[:3].T), _bits(R["spos"])) and np.array_equal(_bits(got[3:].T), _bits(R["snrm"])), name
        _poison(sg, mesh, phi)
        mesh.computeLevelset(phi, c["sigma"], c["cutoff"])
        st = m.lastMeshSdfStats()
        assert (st["sources"], st["binned"]) == (R["counters"]["sources"], R["counters"]["binned"]) and st["rounds"] >= 1, (name, st)
        assert st["rounds"] <= M.tile_rounds(R["pre"], c["dims"], R["P"]["cutoff"])[1]
        _check_field(name, R, pre, phi.to_numpy().reshape(-1))
    assert mesh._sdf_cap == cap and sg._live == live            # buffers reused, scratch returned
    return mesh, phi, sm, sg


@pytest.mark.parametrize("name", M.CASES)
def test_hip_equals_model_equals_fixture(hip_backend, name):
    import manta as m
    _run_case(m, name)


def test_get_levelset_and_argument_checks(hip_backend):
    import manta as m
    c, R = M.case("one"), M.model("one")
    s = _solver(m, c["dims"])
    mesh = s.create(m.Mesh)
    mesh.set_numpy(c["pos"], None, None, c["tris"], None)
    phi = mesh.getLevelset(2.)
    assert isinstance(phi, m.LevelsetGrid) and phi.parent is s
    assert np.array_equal(_bits(phi.to_numpy().reshape(-1)), _bits(R["phi"]))
    keep = phi.to_numpy().tobytes()
    for sigma in (0., -1.):
        with pytest.raises(RuntimeError, match="^Mesh::computeLevelset: sigma must be positive$"):
            mesh.computeLevelset(phi, sigma)
    with pytest.raises(RuntimeError, match="can't convert argument to LevelsetGrid"):
        mesh.computeLevelset(s.create(m.RealGrid), 2.)
    s2 = m.Solver(name="2d", gridSize=m.vec3(8, 8, 1), dim=2)
    with pytest.raises(RuntimeError, match="^Mesh::computeLevelset: 3-D grids only$"):
        mesh.computeLevelset(s2.create(m.LevelsetGrid), 2.)
    with pytest.raises(RuntimeError, match="^Mesh::applyMeshToGrid: 3-D grids only$"):
        mesh.applyMeshToGrid(s2.create(m.RealGrid), value=1.)
    with pytest.raises(RuntimeError, match="^Mesh::getLevelset: 3-D grids only$"):
        s2.create(m.Mesh).getLevelset(2.)
    with pytest.raises(RuntimeError, match="^densityInflowMesh: 3-D grids only$"):
        m.densityInflowMesh(s2.create(m.FlagGrid), s2.create(m.RealGrid), mesh)
    with pytest.raises(RuntimeError, match=r"Shape::applyToGrid\(\): unknown grid type|can't convert argument to GridBase"):
        mesh.applyMeshToGrid(mesh, value=1.)
    with pytest.raises(RuntimeError, match="Argument 'value' is not defined"):
        mesh.applyMeshToGrid(s.create(m.RealGrid))
    s._slab_window = (2, 8)
    try:
        with pytest.raises(RuntimeError, match="^Mesh::computeLevelset: not implemented "):
            mesh.computeLevelset(phi, 2.)
    finally:
        s._slab_window = (0, 0)
    bad = s.create(m.Mesh)
    bad.set_numpy(c["pos"], None, None, [(0, 1, 7)], None)
    with pytest.raises(RuntimeError, match="a triangle names a node outside the mesh's 3 nodes"):
        bad.computeLevelset(phi, 2.)
    bad.set_numpy([(0, 0, 0), (50000, 0, 0), (0, 50000, 0)], None, None, [(0, 1, 2)], None)
    with pytest.raises(RuntimeError, match="edge of 43690 units or more"):
        bad.computeLevelset(phi, 2.)
    assert phi.to_numpy().tobytes() == keep


def _flood(m, dims, v, cutoff):
    import torch
    s = _solver(m, dims) if dims[2] > 1 else None
    lib = m.Solver(name="l", gridSize=m.vec3(4, 4, 4), dim=3).lib if s is None else s.lib
    t = torch.from_numpy(v.copy()).to("cuda")
    stats = torch.full((4,), 123, dtype=torch.int32, device="cuda")
    out = (ctypes.c_int32 * 2)()
    lib.call("mf_meshsdf_flood", dims[0], dims[1], dims[2], ctypes.c_void_p(t.data_ptr()), 1.0, float(cutoff), 1, ctypes.c_void_p(stats.data_ptr()),
             out, None)
    return t.cpu().numpy(), int(out[0])


@pytest.mark.parametrize("name", ["snake", "corner"])
def test_flood_fill_snake_and_corner(hip_backend, name):
    import manta as m
    dims, v, cutoff = M.flood_field(name)
    got, rounds = _flood(m, dims, v, cutoff)
    assert np.array_equal(_bits(got), _bits(M.flood_closure(v, dims, cutoff)[0]))
    print(name, "rounds", rounds)
    assert 1 <= rounds <= M.tile_rounds(v, dims, cutoff)[1]
    if name == "snake":
        assert rounds - 1 > 1           # more than one productive round: the channel leaves and re-enters tiles
    got2, _ = _flood(m, dims, got, cutoff)
    assert np.array_equal(_bits(got2), _bits(got))          # idempotent


def test_flood_fill_random_small_grids(hip_backend):
    import manta as m
    done = 0
    for q in range(200):
        dims, v, cutoff = M.flood_field("rand%d" % q)
        if min(dims[0], dims[1]) < 2 or dims[2] < 2:
            continue
        got, rounds = _flood(m, dims, v, cutoff)
        assert np.array_equal(_bits(got), _bits(M.flood_closure(v, dims, cutoff)[0])), (q, dims, cutoff)
        done += 1
    assert done > 100


def test_sphere_from_create_mesh_closed_and_with_a_triangle_removed(hip_backend):
    import manta as m
    dims = (20, 20, 20)
    s = _solver(m, dims)
    sphere = m.Sphere(parent=s, center=m.vec3(10.2, 9.9, 10.1), radius=6.0)
    mesh, phi = s.create(m.Mesh), s.create(m.LevelsetGrid)
    sphere.computeLevelset().createMesh(mesh)
    pos = mesh.nodes_numpy()[0]
    tris = mesh.tris_numpy()[0]
    assert tris.shape[0] > 500
    for label, tr in (("closed", tris), ("open", np.delete(tris, tris.shape[0] // 2, 0))):
        mesh.set_numpy(pos, None, None, tr, None)
        R = M.mesh_sdf(pos, tr, dims, dims, 1., 2.)
        assert M.margin_ok(R)
        mesh._mesh_sdf(s.lib, "test", phi, 1., 2., flood=False)
        pre = phi.to_numpy().reshape(-1)
        mesh.computeLevelset(phi, 1., 2.)
        got = phi.to_numpy().reshape(-1)
        _check_field("createMesh sphere " + label, R, pre, got)
        if label == "closed":
            f = got.reshape(20, 20, 20)
            assert f[10, 10, 10] == -2.0 and f[0, 0, 0] == 2.0 and (f[8:12, 8:12, 8:12] == -2.0).all()


def test_apply_mesh_to_grid(hip_backend):
    import manta as m
    c, R = M.case("mult"), M.model("mult")
    sm, sg = _solver(m, c["mesh_gs"], "mesh"), _solver(m, c["dims"], "grid")
    mesh = sm.create(m.Mesh)
    mesh.set_numpy(c["pos"], None, None, c["tris"], None)
    n = int(np.prod(c["dims"]))
    rng = np.random.RandomState(4)
    flags_np = rng.choice(np.array([1, 2, 4], np.int32), n, p=[.5, .3, .2])
    flags = sg.create(m.FlagGrid)
    flags.from_numpy(flags_np.reshape(c["dims"][::-1]))
    sdf = R["phi"]
    assert (sdf < 0).any() and ((sdf < 0) & (flags_np == 2)).any()
    for respect in (None, flags):
        fl = None if respect is None else flags_np
        g = sg.create(m.IntGrid)
        g.from_numpy(np.arange(n, dtype=np.int32).reshape(c["dims"][::-1]))
        mesh.applyMeshToGrid(g, respectFlags=respect, value=-5)
        assert np.array_equal(g.to_numpy().reshape(-1), M.apply_mesh_to_grid(np.arange(n, dtype=np.int32), sdf, -5, fl))
        g = sg.create(m.RealGrid)
        base = rng.rand(n).astype(f32)
        g.from_numpy(base.reshape(c["dims"][::-1]))
        mesh.applyMeshToGrid(g, respect, -1., 2., value=0.75)
        assert np.array_equal(_bits(g.to_numpy().reshape(-1)), _bits(M.apply_mesh_to_grid(base, sdf, f32(0.75), fl)))
        g = sg.create(m.MACGrid)
        mesh.applyMeshToGrid(grid=g, respectFlags=respect, value=m.vec3(1, -2, 3.5))
        want = M.apply_mesh_to_grid(np.zeros((3, n), f32), sdf, (1, -2, 3.5), fl)
        got = g.data.view(3, n).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want))
    fg = sg.create(m.FlagGrid)
    mesh.applyMeshToGrid(fg, value=2)
    assert np.array_equal(fg.to_numpy().reshape(-1), np.where(sdf < 0, 2, 0))
    st = m.lastMeshSdfStats()
    assert (st["sources"], st["binned"]) == (R["counters"]["sources"], R["counters"]["binned"])


def test_inflow_plugins(hip_backend):
    import manta as m
    from mantaflow_amd import core
    name = M.INFLOW_CASE
    c = M.case(name)
    s = _solver(m, c["dims"])
    mesh = s.create(m.Mesh)
    mesh.set_numpy(c["pos"], None, None, c["tris"], None)
    flags_np, dens_np = M.inflow_inputs(name)
    flags, dens = s.create(m.FlagGrid), s.create(m.RealGrid)
    flags.from_numpy(flags_np.reshape(c["dims"][::-1]))
    for q, (value, cutoff, sigma) in enumerate(M.INFLOW_ARGS):
        dens.from_numpy(dens_np.reshape(c["dims"][::-1]))
        m.densityInflowMesh(flags=flags, density=dens, mesh=mesh, value=value, cutoff=cutoff, sigma=sigma)
        got = dens.to_numpy().reshape(-1)
        assert np.array_equal(_bits(got), _bits(M.inflow_model(name, q))), q
        assert np.array_equal(M.sha(got), GOLDEN["inflow/%d/sha" % q])          # the reference's own densityInflowMesh
    dens.from_numpy(dens_np.reshape(c["dims"][::-1]))
    m.densityInflowMesh(flags, dens, mesh)                                      # the defaults: value 1, cutoff 7, sigma 0
    assert np.array_equal(_bits(dens.to_numpy().reshape(-1)), _bits(M.inflow_model(name, 0)))
    # densityInflowMeshNoise = computeLevelset(sdf, 1.) + the kernel of densityInflow
    noise = m.NoiseField(parent=s, fixedSeed=265)
    noise.posScale = m.vec3(20)
    noise.clamp, noise.clampNeg, noise.clampPos = True, 0.0, 1.0
    noise.valScale, noise.valOffset = 1.0, 0.75
    sdf = mesh.getLevelset(1.)
    want = s.create(m.RealGrid)
    s.lib.call("mf_density_inflow", flags.sx, flags.sy, flags.sz, flags.ptr, want.ptr, sdf.ptr, core._ptr(noise._tile), noise._params(), 0.8, 0.5,
               s.stream)
    got = s.create(m.RealGrid)
    m.densityInflowMeshNoise(flags, got, noise, mesh, scale=0.8, sigma=0.5)
    w = want.to_numpy()
    assert (w > 0).any() and np.array_equal(_bits(got.to_numpy()), _bits(w))
    assert np.array_equal(_bits(sdf.to_numpy().reshape(-1)), _bits(M.mesh_sdf(c["pos"], c["tris"], c["dims"], c["dims"], 1.)["phi"]))


@pytest.mark.parametrize("name", sorted(M.OBJ_CASES))
def test_obj_scripts_through_load_scale_offset(hip_backend, name):
    """tools/tests/test_0050_meshload.py at res 32 and the set-up of scenes/meshload.py at res 24, as the scripts write them"""
    import manta as m
    fname, res, shift = M.OBJ_CASES[name]
    c, R = M.case(name), M.model(name)
    gs = m.vec3(res, res, res)
    s = m.Solver(name="main", gridSize=gs, dim=3)
    flags, phi, mesh = s.create(m.FlagGrid), s.create(m.LevelsetGrid), s.create(m.Mesh)
    flags.initDomain(boundaryWidth=0)
    mesh.load(os.path.join(M.GOLD, fname))
    mesh.scale(m.vec3(res / 3.0))
    # gs * (Vec3(0.5) + shift) with the reference's fp32 vector arithmetic (the package's vec3 computes in Python floats)
    mesh.offset(m.vec3(*[float(x) for x in M.obj_offset(res, shift)]))
    assert np.array_equal(_bits(mesh.nodes_numpy()[0]), _bits(c["pos"])) and np.array_equal(mesh.tris_numpy()[0], c["tris"])
    mesh._mesh_sdf(s.lib, "test", phi, 2., -1., flood=False)
    pre = phi.to_numpy().reshape(-1)
    mesh.computeLevelset(phi, 2., -1.)
    _check_field(name, R, pre, phi.to_numpy().reshape(-1))
    s.step()
    if name != "torus24":
        return
    # the loop of scenes/meshload.py against the recorded reference run: flags and CG iterations per step identical, the final fields
    # within the project's fp32 parity figure
    import util
    density, vel, pressure = s.create(m.RealGrid), s.create(m.MACGrid), s.create(m.RealGrid)
    flags.initDomain()
    m.setObstacleFlags(flags=flags, phiObs=phi)
    flags.fillGrid()
    assert np.array_equal(flags.to_numpy().reshape(-1), GOLDEN["loop/flags"].astype(np.int32))
    cyl = [float(x) for x in M.loop_cylinder(res)]
    source = s.create(m.Cylinder, center=m.vec3(*cyl[:3]), radius=cyl[3], z=m.vec3(*cyl[4:]))
    iters = []
    for t in range(M.LOOP_STEPS):
        source.applyToGrid(grid=density, value=1.)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=density, order=2)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2, strength=1.0)
        m.setWallBcs(flags=flags, vel=vel)
        m.addBuoyancy(density=density, vel=vel, gravity=m.vec3(0, -1e-3, 0), flags=flags)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure)
        iters.append(m.lastCgStats()["iterations"])
        s.step()
    assert iters == GOLDEN["loop/iterations"].tolist()
    s.sync()
    for key, got in (("density", density.to_numpy().reshape(-1)), ("vel", vel.data.cpu().numpy()), ("pressure", pressure.to_numpy().reshape(-1))):
        e = util.rel_err(got, GOLDEN["loop/" + key])
        print("meshload loop %s: relative error %g" % (key, e))
        assert e <= 1e-5, (key, e)
