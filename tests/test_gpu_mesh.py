"""GPU: surface meshes through the package on the HIP backend against the numpy model and the recorded reference
(tests/golden/mesh.npz; how each array was produced: tools/record_mesh.py; arrays of more than mesh_model.FULL_LIMIT elements are in
the fixture as SHA-256 digests, so the device result is also compared, word by word, with the model's array).

createMesh: HIP = model = reference bit for bit -- node count, triangle count, every node's position and normal, every triangle index,
all flags zero -- on every fixture case: the 256 sign configurations of a cell, invalid-time cells that pass ownership on, phi == -1e-4f
at a corner, the three branches of getNormalized, empty meshes, rows of 65 and columns of 70 cells, and 33x31x29 (28 160 cells: the scans
span several blocks).  The mesh holds a larger previous mesh of NaN and -1 and the solver's pool scratch is filled with garbage before the
call; each case is meshed twice in a row on one solver."""
import gzip
import os
import zlib

import numpy as np
import pytest

import mesh_model as M
import util

pytestmark = pytest.mark.gpu
GOLD = os.path.dirname(M.GOLDEN)
GOLDEN = np.load(M.GOLDEN)
f32 = np.float32


def _solver(m, dims, dt=1.0):
    s = m.Solver(name="t", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)
    s.timestep = dt
    return s


def _poison_pool(s, n=5):
    """the next scratch grids createMesh takes from the solver's pool hold garbage"""
    import torch
    for q in range(n):
        s._pool.setdefault("int", []).append(torch.full((s.ncells,), 0x7f7f7f7f - q, dtype=torch.int32, device=s.device))


def _poison_mesh(mesh, nodes, tris):
    """a larger previous mesh of NaN positions and normals, -1 flags and -1 triangle indices"""
    mesh.set_numpy(np.full((nodes, 3), np.nan, f32), np.full((nodes, 3), np.nan, f32), np.full(nodes, -1, np.int32),
                   np.full((tris, 3), -1, np.int32), np.full(tris, -1, np.int32))


def _read(mesh):
    pos, normal, nflags = mesh.nodes_numpy()
    tris, tflags = mesh.tris_numpy()
    assert not nflags.any() and not tflags.any(), "node / triangle flags are not all zero"
    return {"pos": pos, "normal": normal, "tris": tris}


def _check(key, got, model, fixture=True):
    for k in ("pos", "normal", "tris"):
        a, b = got[k], model[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (key, k, a.shape, b.shape)
        d = a.view(np.uint32) != b.view(np.uint32)
        assert not d.any(), "%s/%s vs model: %d of %d words differ, first at %s" % (key, k, int(d.sum()), d.size, np.argwhere(d)[0])
    if fixture:
        msg = M.mesh_same_as_fixture(GOLDEN, key, got)
        assert msg is None, msg


def test_create_mesh_all_256_sign_configurations(hip_backend):
    import manta as m
    s = _solver(m, (3, 3, 3))
    phi, mesh = s.create(m.LevelsetGrid), s.create(m.Mesh)
    _poison_pool(s)
    _poison_mesh(mesh, 200, 300)
    for c in range(256):
        name = "cfg%03d" % c
        phi.from_numpy(M.case_phi(name))
        phi.createMesh(mesh)
        _check("create/" + name, _read(mesh), M.model_mesh(name)[0])
    assert mesh.ncap == 200 and mesh.tcap == 300              # the buffers were reused throughout


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_create_mesh_cases(hip_backend, name):
    import manta as m
    data = M.case_phi(name)
    model = M.model_mesh(name)[0]
    nn, nt = model["pos"].shape[0], model["tris"].shape[0]
    s = _solver(m, data.shape[::-1])
    phi, mesh = s.create(m.LevelsetGrid), s.create(m.Mesh)
    phi.from_numpy(data)
    _poison_pool(s)
    live = s._live
    _poison_mesh(mesh, nn + 100, nt + 100)
    phi.createMesh(mesh)
    _check("create/" + name, _read(mesh), model)
    assert (mesh.numNodes(), mesh.numTris(), mesh.ncap, mesh.tcap) == (nn, nt, nn + 100, nt + 100)
    assert s._live == live                                   # the scratch went back to the pool
    phi.createMesh(mesh)                                     # a second call in a row, on the mesh the first one left
    _check("create/" + name, _read(mesh), model)
    other = s.create(m.Mesh)                                 # and into empty buffers, which have to grow
    phi.createMesh(other)
    _check("create/" + name, _read(other), model)
    assert np.array_equal(phi.to_numpy(), data)              # phi is read only


def test_create_mesh_random_grids(hip_backend):
    import manta as m
    r = np.random.RandomState(77)
    for q in range(6):
        dims = tuple(int(v) for v in r.randint(3, 12, 3))
        data = r.uniform(-1, 1, dims[::-1]).astype(f32)
        data[r.uniform(size=data.shape) < 0.03] = M.INVALID
        data[tuple(r.randint(0, v) for v in data.shape)] = -M.ISO
        cnt = {}
        model = M.create_mesh(data, cnt)
        s = _solver(m, dims)
        phi, mesh = s.create(m.LevelsetGrid), s.create(m.Mesh)
        phi.from_numpy(data)
        _poison_pool(s)
        phi.createMesh(mesh)
        _check("random %d %s" % (q, dims), _read(mesh), model, fixture=False)
        print("random grid", dims, model["pos"].shape[0], "nodes", cnt)


def test_create_mesh_refusals(hip_backend):
    import manta as m
    s2 = _solver(m, (8, 8, 1))
    mesh2 = s2.create(m.Mesh)
    mesh2.set_numpy(np.ones((3, 3), f32))
    with pytest.raises(RuntimeError, match="Only 3D grids supported so far"):
        s2.create(m.LevelsetGrid).createMesh(mesh2)
    assert mesh2.numNodes() == 3
    s = _solver(m, (6, 6, 2))
    with pytest.raises(RuntimeError, match="thinner than 3 cells"):
        s.create(m.LevelsetGrid).createMesh(s.create(m.Mesh))
    with pytest.raises(RuntimeError, match="can't convert argument to Mesh"):
        s.create(m.LevelsetGrid).createMesh(None)


@pytest.mark.parametrize("n", M.ADV_SIZES)
def test_advect_in_grid(hip_backend, n):
    import manta as m
    s = _solver(m, M.ADV_DIMS, M.ADV_DT)
    sx, sy, sz = M.ADV_DIMS
    velv, pos, nflags = M.advect_inputs(n)
    flags, vel = s.create(m.FlagGrid), s.create(m.MACGrid)
    vel.from_numpy(np.ascontiguousarray(velv.reshape(3, sz, sy, sx).transpose(1, 2, 3, 0)))
    for mode in (m.IntEuler, m.IntRK2, m.IntRK4):
        mesh = s.create(m.Mesh)
        mesh.set_numpy(pos.T, None, nflags)
        mesh.advectInGrid(flags, vel, mode)
        got, _, fl = mesh.nodes_numpy()
        model = np.ascontiguousarray(M.advect_nodes(M.ADV_DIMS, velv, pos, nflags, M.ADV_DT, mode).T)
        assert got.tobytes() == model.tobytes(), (n, mode)
        msg = M.same_as_fixture(GOLDEN, "adv/%d/%d" % (n, mode), got)
        assert msg is None, msg
        assert np.array_equal(fl, nflags)
    with pytest.raises(RuntimeError, match="unknown integration type"):
        mesh.advectInGrid(flags, vel, 3)


def test_node_transforms(hip_backend):
    import manta as m
    from mantaflow_amd import core
    s = _solver(m, (8, 8, 8))
    pos = M.xf_inputs()

    def fresh(p=pos):
        mesh = s.create(m.Mesh)
        mesh.set_numpy(p)
        mesh._reserve_nodes(p.shape[0] + 37)                 # a stride that is not the node count
        return mesh
    me = fresh()
    me.scale(m.vec3(*M.XF_SCALE))
    msg = M.same_as_fixture(GOLDEN, "xf/scale", me.nodes_numpy()[0])
    assert msg is None, msg
    me = fresh()
    me.offset(m.vec3(*M.XF_OFFSET))
    msg = M.same_as_fixture(GOLDEN, "xf/offset", me.nodes_numpy()[0])
    assert msg is None, msg
    me = fresh()
    me.save_pos()
    me.scale(m.vec3(*M.XF_SCALE))
    me.load_pos()
    msg = M.same_as_fixture(GOLDEN, "xf/savepos", me.nodes_numpy()[0])
    assert msg is None, msg
    me.set_numpy(pos[:-1])
    with pytest.raises(RuntimeError, match="# of mesh nodes has changed"):
        me.load_pos()
    for q, th in enumerate(M.ROT_THETAS):
        me = fresh()
        me.rotate(m.vec3(*th))
        got = me.nodes_numpy()[0]
        # the kernel's arithmetic against the model fed the library's own scalars (this machine's C library need not be the recorder's)
        sc = np.array([core._c_sincos(s.lib, float(f32(t))) for t in th], f32)
        model = np.ascontiguousarray(M.rotate(np.ascontiguousarray(pos.T), th, sc).T)
        assert got.tobytes() == model.tobytes(), q
        if np.array_equal(sc.view(np.uint32), GOLDEN["xf/rotate/%d/scalars" % q].view(np.uint32)):
            msg = M.same_as_fixture(GOLDEN, "xf/rotate/%d" % q, got)
            assert msg is None, msg
    for n in (0, 1, 63, 64, 65):
        me = fresh(pos[:n])
        me.scale(m.vec3(*M.XF_SCALE))
        me.rotate(m.vec3(0.5, 0, 0))
        me.offset(m.vec3(*M.XF_OFFSET))
        assert me.numNodes() == n and np.isfinite(me.nodes_numpy()[0]).all()


def test_save_after_a_device_create_mesh_writes_the_reference_bytes(hip_backend, tmp_path):
    import manta as m
    s = _solver(m, M.SAVE_DIMS)
    phi, mesh = s.create(m.LevelsetGrid), s.create(m.Mesh)
    phi.from_numpy(M.case_phi(M.SAVE_CASE))
    phi.createMesh(mesh)
    mesh.save(str(tmp_path / "surface_0001.obj"))
    assert open(tmp_path / "surface_0001.obj", "rb").read() == open(os.path.join(GOLD, "mesh_small.obj"), "rb").read()
    mesh.save(str(tmp_path / "surface_0001.bobj.gz"))
    assert gzip.open(tmp_path / "surface_0001.bobj.gz").read() == gzip.open(os.path.join(GOLD, "mesh_small.bobj.gz")).read()
    msg = M.same_as_fixture(GOLDEN, "save/bobj.gz/normal_after", mesh.nodes_numpy()[1])      # the normals went back to the device
    assert msg is None, msg
    other = s.create(m.Mesh)
    other.load(str(tmp_path / "surface_0001.bobj.gz"))
    msg = M.mesh_same_as_fixture(GOLDEN, "load/bobj.gz/00", _read(other))
    assert msg is None, msg


def test_flip_loop_meshes_equal_the_recorded_reference_run(hip_backend):
    """scenes/flip02_surface.py's dam break at 32^3, 8 steps, with improvedParticleLevelset; every step a copy of phi gets setBound(0, 1)
    and createMesh, as scenes/flip03_gen.py does it.  Node and triangle counts per step and the final mesh against the recorded reference
    run; every step's mesh against the model on the device's own phi; then the final mesh advected 3 steps with RK4."""
    import manta as m
    import partls_model as PM
    st, counts, crcs = {}, [], []

    def after_levelset(t, phi, pp, pindex, gpi, flags):
        s = phi.parent
        if not st:
            st.update(mesh=s.create(m.Mesh), phi=s.create(m.LevelsetGrid), flags=flags, s=s)
        crcs.append(zlib.crc32(np.ascontiguousarray(phi.to_numpy(), f32).tobytes()) & 0xffffffff)
        st["phi"].copyFrom(phi)
        st["phi"].setBound(0., 1)
        st["phi"].createMesh(st["mesh"])
        counts.append([st["mesh"].numNodes(), st["mesh"].numTris()])
        if t in (0, M.LOOP_STEPS - 1):
            _check("loop step %d" % t, _read(st["mesh"]), M.create_mesh(st["phi"].to_numpy()), fixture=False)

    out = PM.flip_loop(m, True, res=M.LOOP_RES, steps=M.LOOP_STEPS, after_levelset=after_levelset)
    print("nodes / triangles per step:", counts)
    print("phi equals the reference run's per step:", [int(a) == int(b) for a, b in zip(crcs, GOLDEN["loop/crc"])])
    assert np.array_equal(np.array(counts, np.int64), GOLDEN["loop/counts"]), (counts, GOLDEN["loop/counts"].tolist())
    mesh, s = st["mesh"], st["s"]
    final = _read(mesh)
    msg = M.mesh_same_as_fixture(GOLDEN, "loop/mesh", final)
    assert msg is None, msg
    vel = s.create(m.MACGrid)
    vel.from_numpy(out["vel"])
    for _ in range(M.LOOP_ADV_STEPS):
        mesh.advectInGrid(st["flags"], vel, m.IntRK4)
    adv = mesh.nodes_numpy()[0]
    msg = M.same_as_fixture(GOLDEN, "loop/adv", adv)
    assert msg is None, msg
    n = M.LOOP_RES ** 3
    velv = np.ascontiguousarray(out["vel"].reshape(n, 3).T)
    p = np.ascontiguousarray(final["pos"].T)
    for _ in range(M.LOOP_ADV_STEPS):
        p = M.advect_nodes((M.LOOP_RES,) * 3, velv, p, np.zeros(p.shape[1], np.int32), s.getDt(), M.INT_RK4)
    assert adv.tobytes() == np.ascontiguousarray(p.T).tobytes()
