"""GPU: the mesh connectivity tables, smoothMesh and killSmallComponents through the package on the HIP backend against the numpy model
(tests/meshops_model.py) and the recorded reference (tests/golden/meshops.npz; how each array was produced: tools/record_meshops.py;
arrays of more than mesh_model.FULL_LIMIT elements are digests there, so the device result is also compared with the model's array).

Every case is HIP = model = reference bit for bit: `opposite`, both CSR tables, positions, normals, flags, triangles, counts.  The mesh
buffers hold a larger previous mesh of NaN and -1 beyond the case's nodes and triangles, the solver's pool scratch is filled with garbage,
and each call is made twice in a row.  The eight fp64 sums of smoothMesh stay within 2 * gamma_{T-1} * sum|term| of the model's serial
sums, and the per-triangle terms are bit-identical through the kernel-level entry."""
import ctypes
import gzip
import os

import numpy as np
import pytest

import meshops_model as M

pytestmark = pytest.mark.gpu
GOLDEN = np.load(M.GOLDEN)
f32, i32 = np.float32, np.int32
DIMS = (24, 24, 24)


def _solver(m, dims=DIMS, dt=1.0, dim=3):
    s = m.Solver(name="t", gridSize=m.vec3(*dims), dim=dim)
    s.timestep = dt
    return s


def _poison_pool(s, n=3):
    import torch
    for q in range(n):
        s._pool.setdefault("int", []).append(torch.full((s.ncells,), 0x7f7f7f7f - q, dtype=torch.int32, device=s.device))
        s._pool.setdefault("vec", []).append(torch.full((3 * s.ncells,), float("nan"), dtype=torch.float32, device=s.device))


def _load(mesh, model, extra=57):
    """the case in buffers that a larger previous mesh of NaN and -1 has filled"""
    n, t = model["pos"].shape[0] + extra, model["tris"].shape[0] + extra
    mesh.set_numpy(np.full((n, 3), np.nan, f32), np.full((n, 3), np.nan, f32), np.full(n, -1, i32), np.full((t, 3), -1, i32), np.full(t, -1, i32))
    mesh.set_numpy(model["pos"], model["normal"], model["flags"], model["tris"], model["tflags"])
    assert mesh.ncap >= n and mesh.tcap >= t and mesh.ncap > mesh.numNodes() and mesh.tcap > mesh.numTris()


def _read(mesh):
    pos, normal, flags = mesh.nodes_numpy()
    tris, tflags = mesh.tris_numpy()
    return {"pos": pos, "normal": normal, "flags": flags, "tris": tris, "tflags": tflags}


def _same_mesh(tag, got, want):
    for k in M.MESH_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (tag, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), "%s/%s differs from the model" % (tag, k)


def _same_conn(tag, mesh, model, fixture=None):
    want = M.connectivity(tag, model)
    off, nodes, toff, tris = mesh.ring_numpy()
    got = {"opposite": mesh.corners_numpy(), "nodeOff": off, "nodes": nodes, "triOff": toff, "tris": tris}
    for k, v in got.items():
        assert v.dtype == i32 and v.shape == want[k].shape and np.array_equal(v, want[k]), (tag, k)
        if fixture:
            msg = M.same_as_fixture(GOLDEN, "conn/%s/%s" % (fixture, k), v)
            assert msg is None, msg
    return want


@pytest.mark.parametrize("name", sorted(M.CONNECTIVITY_CASES))
def test_connectivity_cases(hip_backend, name):
    import manta as m
    model = M.CONNECTIVITY_CASES[name]()
    s = _solver(m)
    mesh = s.create(m.Mesh)
    _poison_pool(s)
    live = s._live
    _load(mesh, model)
    before = _read(mesh)
    opp = mesh.corners_numpy()
    st = m.lastMeshOpsStats()
    want = _same_conn(name, mesh, model, fixture=name)
    assert np.array_equal(opp, want["opposite"]) and (st["singletons"], st["multi"], st["rebuilt"]) == (0, want["multi"], True)
    assert m.lastMeshOpsStats()["rebuilt"] is False and m.lastMeshOpsStats()["multi"] == want["multi"]      # _same_conn reused the tables
    _same_mesh(name, _read(mesh), before)                    # the mesh is read only
    assert s._live == live                                   # the scratch went back to the pool
    _load(mesh, model)                                       # a second build in a row, into the same buffers
    _same_conn(name, mesh, model, fixture=name)


@pytest.mark.parametrize("name", sorted(M.REFUSED_CASES))
def test_connectivity_refusals_leave_mesh_and_cache(hip_backend, name):
    import manta as m
    make, msg = M.REFUSED_CASES[name]
    s = _solver(m)
    mesh = s.create(m.Mesh)
    _load(mesh, M.bipyramid(5))
    mesh.corners_numpy()
    cache, gen = mesh._conn, mesh._conn_gen
    _load(mesh, make())
    before = _read(mesh)
    for who, call in (("Mesh::corners_numpy", mesh.corners_numpy), ("Mesh::ring_numpy", mesh.ring_numpy),
                      ("smoothMesh", lambda: m.smoothMesh(mesh, 0.5)), ("killSmallComponents", lambda: m.killSmallComponents(mesh))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == (msg % who if "%s" in msg else msg)
    _same_mesh(name, _read(mesh), before)
    assert mesh._conn is cache and mesh._conn_gen == gen and gen != mesh._topo_gen


@pytest.mark.parametrize("name", sorted(M.SMOOTH_CASES))
def test_smooth_cases(hip_backend, name):
    import manta as m
    model, dt, strength, steps, minLength = M.SMOOTH_CASES[name]()
    s = _solver(m, dt=dt)
    mesh = s.create(m.Mesh)
    _poison_pool(s)
    live = s._live
    _load(mesh, model)
    want, sums = model, None
    for rep in range(2):                                     # twice in a row: the second call smooths what the first one left
        terms = []
        want, sums = M.smooth_mesh(want, dt, strength, steps, minLength, terms=terms)
        m.smoothMesh(mesh, strength, steps, minLength)
        st = m.lastMeshOpsStats()
        assert st["rebuilt"] is (rep == 0)
        got = _read(mesh)
        if rep == 0:
            msg = M.same_as_fixture(GOLDEN, "smooth/%s/pos" % name, got["pos"])
            assert msg is None, msg
        _same_mesh("%s/%d" % (name, rep), got, want)
        dev, bound = np.array(st["sums"]), np.stack([M.sum_bound(t) for t in terms])
        print(name, rep, "sums: device - serial", (dev - sums).tolist(), "bound", bound.tolist())
        assert (np.abs(dev - sums) <= bound).all()           # all eight sums
    assert s._live == live


@pytest.mark.parametrize("name", ["sphere17", "apex300", "two"])
def test_volume_terms_and_sums_through_the_kernel_level_entries(hip_backend, name):
    import manta as m
    import torch
    from mantaflow_amd.core import _ptr
    model = M.SMOOTH_CASES[name]()[0]
    s = _solver(m)
    mesh = s.create(m.Mesh)
    _load(mesh, model)
    t = model["tris"].shape[0]
    terms = torch.full((4 * t,), float("nan"), dtype=torch.float64, device=s.device)
    s.lib.call("mf_meshops_volume_terms", t, mesh.tcap, _ptr(mesh.tri), mesh.nn, mesh.ncap, _ptr(mesh.pos), _ptr(terms), s.stream)
    s.sync()
    want = M.volume_terms(model["pos"], model["tris"])
    assert terms.cpu().numpy().reshape(4, t).T.tobytes() == want.tobytes()            # bit-identical per triangle
    need = ctypes.c_int64(0)
    s.lib.call("mf_meshops_tmp_bytes", t, mesh.nn, ctypes.byref(need))
    tmp = torch.full((need.value,), 0x5a, dtype=torch.uint8, device=s.device)
    runs = []
    for _ in range(2):
        out = (ctypes.c_double * 4)()
        s.lib.call("mf_meshops_volume_sums", t, mesh.tcap, _ptr(mesh.tri), mesh.nn, mesh.ncap, _ptr(mesh.pos), _ptr(tmp), need.value, out, s.stream)
        runs.append(np.array(out))
    assert runs[0].tobytes() == runs[1].tobytes()                                      # a fixed tree: the same bits from run to run
    assert (np.abs(runs[0] - M.serial_sums(want)) <= M.sum_bound(want)).all()


@pytest.mark.parametrize("name", sorted(M.KILL_CASES))
def test_kill_cases(hip_backend, name, capsys):
    import manta as m
    model, elements = M.KILL_CASES[name]()
    want, stats = M.kill_small_components(model, elements)
    s = _solver(m)
    mesh = s.create(m.Mesh)
    _poison_pool(s)
    live = s._live
    _load(mesh, model)
    mesh.corners_numpy()
    cache = mesh._conn
    capsys.readouterr()
    if elements == 10:
        m.killSmallComponents(mesh)                          # the default
    else:
        m.killSmallComponents(mesh, elements)
    text = capsys.readouterr().out
    st = m.lastMeshOpsStats()
    got = _read(mesh)
    _same_mesh(name, got, want)
    msg = M.mesh_same_as_fixture(GOLDEN, "kill/" + name, got)
    assert msg is None, msg
    assert (st["components"], st["tris"], st["nodes"]) == (stats["components"], stats["tris"], stats["nodes"]) and st["rounds"] >= 1
    assert s._live == live
    if stats["tris"]:
        assert text == M.kill_message(stats) + "\n" == GOLDEN["kill/%s/message" % name].tobytes().decode() + "\n"
        assert mesh._conn_gen != mesh._topo_gen              # the tables are those of the old triangle list
        if want["tris"].shape[0]:
            _same_conn(name, mesh, want)
            assert mesh._conn is not cache
    else:
        assert text == "" and mesh._conn is cache and mesh._conn_gen == mesh._topo_gen
    # a second call in a row, on the mesh the first one left: nothing is small any more
    again, stats2 = M.kill_small_components(want, elements)
    m.killSmallComponents(mesh, elements)
    assert stats2["tris"] == 0 and capsys.readouterr().out == ""
    _same_mesh(name + "/again", _read(mesh), again)


@pytest.mark.parametrize("name", sorted(M.KILL_REFUSED))
def test_kill_refusals_leave_the_mesh(hip_backend, name, capsys):
    import manta as m
    make, msg = M.KILL_REFUSED[name]
    model, elements = make()
    s = _solver(m)
    mesh = s.create(m.Mesh)
    _load(mesh, model)
    before = _read(mesh)
    gen = mesh._topo_gen
    with pytest.raises(RuntimeError) as e:
        m.killSmallComponents(mesh, elements)
    assert str(e.value) == msg and capsys.readouterr().out == ""
    _same_mesh(name, _read(mesh), before)
    assert mesh._topo_gen == gen


def test_cache_is_kept_by_position_changes_and_dropped_by_topology_changes(hip_backend, tmp_path):
    import manta as m
    phi_np = M.two_blobs(24)
    s = _solver(m, dt=0.5)
    phi, mesh, flags, vel = s.create(m.LevelsetGrid), s.create(m.Mesh), s.create(m.FlagGrid), s.create(m.MACGrid)
    flags.initDomain()
    flags.fillGrid()
    vel.setConst(m.vec3(0.25, -0.125, 0.5))
    phi.from_numpy(phi_np)
    rebuilt = lambda: (mesh.corners_numpy(), m.lastMeshOpsStats()["rebuilt"])[1]
    phi.createMesh(mesh)
    assert rebuilt() is True and rebuilt() is False
    mesh.advectInGrid(flags, vel, m.IntRK4)
    mesh.scale(m.vec3(1, 1, 1))
    assert rebuilt() is False
    m.smoothMesh(mesh, 0.5)
    assert m.lastMeshOpsStats()["rebuilt"] is False
    phi.createMesh(mesh)
    assert rebuilt() is True
    mesh.save(str(tmp_path / "a.bobj.gz"))
    assert rebuilt() is False
    mesh.load(str(tmp_path / "a.bobj.gz"))
    assert rebuilt() is True
    m.killSmallComponents(mesh)
    assert m.lastMeshOpsStats()["tris"] > 0 and rebuilt() is True
    mesh.clear()
    assert rebuilt() is True and mesh.corners_numpy().size == 0
    # a 2-D solver: the mesh operations do not look at the grid
    s2 = _solver(m, (16, 16, 1), dim=2)
    flat = s2.create(m.Mesh)
    _load(flat, M.bipyramid(7))
    _same_conn("2d", flat, M.bipyramid(7))


def test_larger_mesh_spans_many_blocks(hip_backend, capsys):
    """6 000 triangles with two small components interleaved: sorts, scans and the labelling over several blocks and rounds"""
    import manta as m
    model = M.join([M.sphere(40), M.tetrahedron(1, (2, 2, 2)), M.bipyramid(4, 2, (37, 37, 37))], seed=21, tri_seed=22)
    assert model["tris"].shape[0] > 5000
    s = _solver(m, dt=0.5)
    mesh = s.create(m.Mesh)
    _poison_pool(s)
    _load(mesh, model)
    _same_conn("large", mesh, model)
    want, stats = M.kill_small_components(model, 10)
    m.killSmallComponents(mesh)
    st = m.lastMeshOpsStats()
    assert (st["components"], st["tris"], st["nodes"]) == (3, 12, 10) == (stats["components"], stats["tris"], stats["nodes"])
    print("labelling rounds:", st["rounds"])
    _same_mesh("large/kill", _read(mesh), want)
    terms = []
    want, sums = M.smooth_mesh(want, 0.5, 0.6, 2, terms=terms)
    m.smoothMesh(mesh, 0.6, 2)
    dev = np.array(m.lastMeshOpsStats()["sums"])
    assert (np.abs(dev - sums) <= np.stack([M.sum_bound(t) for t in terms])).all()
    _same_mesh("large/smooth", _read(mesh), want)


def test_pipeline_equals_the_recorded_reference_run(hip_backend, tmp_path, capsys):
    """createMesh on a 24^3 level set of two blobs -> killSmallComponents -> smoothMesh(steps=3) -> save: the reference's file, by
    decompressed bytes"""
    import manta as m
    s = _solver(m, dt=0.5)
    phi, mesh = s.create(m.LevelsetGrid), s.create(m.Mesh)
    phi.from_numpy(M.two_blobs(24))
    phi.createMesh(mesh)
    counts = [mesh.numNodes(), mesh.numTris()]
    m.killSmallComponents(mesh)
    m.smoothMesh(mesh, 0.6, steps=3)
    assert counts + [mesh.numNodes(), mesh.numTris()] == GOLDEN["pipeline/counts"].tolist()
    mesh.save(str(tmp_path / "p.bobj.gz"))
    assert gzip.open(tmp_path / "p.bobj.gz").read() == gzip.open(os.path.join(os.path.dirname(M.GOLDEN), "meshops_pipeline.bobj.gz")).read()
