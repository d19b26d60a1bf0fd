"""GPU: vortex sheets through the opt-in module on the HIP backend against the recorded reference (tests/golden/vsheet.npz; how each array
was produced: tools/record_vsheet.py) and the numpy model (tests/vsheet_model.py).

Every arithmetic stage -- calcVorticity, reinitTexCoords, meshSmokeInflow, vorticitySource, the smoothing passes from a given table,
texcoordInflow -- is HIP = model = reference bit for bit.  The smoothing weights are held to the reference within
vsheet_model.WEIGHT_ULPS and to the model bit for bit but for at most one weight per case (the device's and the host's fp64 exp may round one
fp32 result differently).  The mesh buffers hold a larger previous mesh of NaN and -1 beyond the case, channels and
outputs are pre-filled with NaN, and the solver's pool scratch is filled with garbage."""
import ctypes

import numpy as np
import pytest

import mesh_model as MM
import meshops_model as MO
import vsheet_model as M

pytestmark = pytest.mark.gpu
G = M.golden()
f32, i32 = np.float32, np.int32
NAN = float("nan")


def _solver(m, dims=M.DIMS, dt=M.DT, dim=3):
    s = m.Solver(name="t", gridSize=m.vec3(*dims), dim=dim)
    s.timestep = dt
    return s


def _poison_pool(s, n=4):
    import torch
    for q in range(n):
        s._pool.setdefault("int", []).append(torch.full((s.ncells,), 0x7f7f7f7f - q, dtype=torch.int32, device=s.device))
        s._pool.setdefault("vec", []).append(torch.full((3 * s.ncells,), NAN, dtype=torch.float32, device=s.device))


def _sheet(m, s, model, extra=57):
    """the case in buffers that a larger previous mesh of NaN and -1 has filled, channels of NaN behind the defaults"""
    from mantaflow_amd.vortexsheet import VortexSheetMesh
    mesh = s.create(VortexSheetMesh)
    n, t = model["pos"].shape[0] + extra, model["tris"].shape[0] + extra
    mesh.set_numpy(np.full((n, 3), NAN, f32), np.full((n, 3), NAN, f32), np.full(n, -1, i32), np.full((t, 3), -1, i32), np.full(t, -1, i32))
    mesh._channels("test")
    for ch in mesh._ch.values():
        ch.fill_(NAN)
    mesh.set_numpy(model["pos"], model["normal"], model["flags"], model["tris"], model["tflags"])
    assert mesh.ncap > mesh.numNodes() and mesh.tcap > mesh.numTris()
    return mesh


def _same(tag, got, want):
    """the same bits; a NaN equals a NaN whatever its sign and payload (0 / 0 is the negative default NaN on the reference's host and
    the positive one on the device: not a value)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype == f32:
        got, want = np.where(np.isnan(got), f32(NAN), got), np.where(np.isnan(want), f32(NAN), want)
    assert got.tobytes() == want.tobytes(), "%s: %d of %d words differ" % (tag, int((got.view("u4") != want.view("u4")).sum()), got.size)


def _shape(m, s, shape):
    if shape[0] == "box":
        return m.Box(parent=s, p0=m.vec3(*shape[1]), p1=m.vec3(*shape[2]))
    return m.Sphere(parent=s, center=m.vec3(*shape[1]), radius=shape[2])


def _mac(m, s, planes):
    import torch
    g = s.create(m.MACGrid)
    g.data.copy_(torch.from_numpy(np.ascontiguousarray(planes.reshape(-1))).to(g.data.device))
    return g


def _dev(s, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(s.device)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def soup(T, seed):
    """T seeded triangles over seeded nodes, no connectivity: for the per-triangle stages at the launch edges"""
    r = M._rs("vs-soup", T, seed)
    n = max(3, T // 2 + 3)
    tris = np.stack([r.permutation(n)[:3] for _ in range(T)]).reshape(T, 3) if T else np.zeros((0, 3))
    m = MO.mesh(r.uniform(1.5, 14.0, (n, 3)), tris)
    m["flags"] = np.where(r.uniform(size=n) < 0.2, 1, 0).astype(i32)
    return m


def _stage_case(m, vs, name, model, fixture):
    s = _solver(m)
    _poison_pool(s)
    nt = model["tris"].shape[0]
    st = M.sheet_state(name, nt)
    mesh = _sheet(m, s, model)
    want = M.default_sheet(nt)
    got = mesh.sheet_numpy()
    for k in M.DEFAULTS:                                          # the rebuild left the reference's defaults over the NaN
        _same("defaults/" + k, got[k], want[k])
    assert not np.concatenate(mesh.tex_numpy()).any() and not np.concatenate(mesh.turb_numpy()).any()
    # calcVorticity
    mesh.set_sheet_numpy(**dict(st, vorticity=np.full((nt, 3), NAN, f32)))
    mesh.calcVorticity()
    got = mesh.sheet_numpy()
    v, smoke = M.calc_vorticity(model, st["circulation"])
    _same("calc/vorticity", got["vorticity"], v)
    _same("calc/smokeAmount", got["smokeAmount"], smoke)
    for k in ("vorticitySmoothed", "circulation", "smokeParticles"):
        _same("calc leaves " + k, got[k], st[k])
    if fixture:
        _same("calc/vorticity", got["vorticity"], G["calc/%s/vorticity" % name])
        _same("calc/smokeAmount", got["smokeAmount"], G["calc/%s/smokeAmount" % name])
    # meshSmokeInflow
    for sname, shape in M.SMOKE_SHAPES.items():
        mesh.set_sheet_numpy(**st)
        vs.meshSmokeInflow(mesh, _shape(m, s, shape), 0.37)
        got = mesh.sheet_numpy()["smokeAmount"]
        _same("smoke/" + sname, got, M.smoke_inflow(model, shape, 0.37, st["smokeAmount"]))
        if fixture:
            _same("smoke/" + sname, got, G["smoke/%s/%s" % (name, sname)])
    # vorticitySource
    vel, old = M.mac_grid("src-" + name), M.mac_grid("src-old-" + name)
    gv, go = _mac(m, s, vel), _mac(m, s, old)
    live = s._live
    for vname, (with_vel, maxAmount, mult, scale) in M.SOURCE_VARIANTS.items():
        mesh.set_sheet_numpy(**st)
        vs.vorticitySource(mesh, m.vec3(*M.GRAVITY), gv if with_vel else None, go if with_vel else None, scale=scale, maxAmount=maxAmount, mult=mult)
        got = mesh.sheet_numpy()
        w, vn = M.vorticity_source(model, st["vorticity"], M.GRAVITY, M.DIMS, M.DT, vel if with_vel else None, old if with_vel else None, scale,
                                   maxAmount, mult)
        _same("source/" + vname, got["vorticity"], w)
        if fixture:
            _same("source/" + vname, got["vorticity"], G["source/%s/%s" % (name, vname)])
        stats = vs.lastVortexSheetStats()["source"]
        if nt:
            assert stats["max"] == float(vn.max()), vname                                  # exact
            mean = float(vn.astype(np.float64).sum() / nt)
            assert abs(stats["mean"] - mean) <= (2 * nt + 2) * 2.0 ** -53 * mean, vname        # two fp64 sums of other orders, one division
        else:
            assert stats["max"] == 0.0 and np.isnan(stats["mean"])
    pos, _, fl = mesh.nodes_numpy()
    _same("the mesh is read only", pos, model["pos"])
    assert s._live == live                                       # the acceleration grid and the norms went back to the pool


@pytest.mark.parametrize("name", sorted(M.MESHES))
def test_recorded_stage_cases(hip_backend, name):
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    _stage_case(m, vs, name, M.with_fixed(M.MESHES[name](), name), True)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_stages_equal_the_model_at_the_launch_edges(hip_backend, T):
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    _stage_case(m, vs, "soup%d" % T, soup(T, 1), False)


def _weights_entry(s, mesh, opp, sigma):
    import torch
    nt = mesh.nt
    w = torch.full((max(3 * nt, 1),), NAN, dtype=torch.float32, device=s.device)
    idx = torch.full((max(3 * nt, 1),), -7, dtype=torch.int32, device=s.device)
    table = _dev(s, opp.astype(i32))
    s.lib.call("mf_vsheet_smooth_weights", *(mesh._mesh_args() + (_p(table), float(M.smooth_mult(sigma)), _p(w), _p(idx), s.stream)))
    s.sync()
    return w[:3 * nt].cpu().numpy(), idx[:3 * nt].cpu().numpy()


def _iterate_entry(s, mesh, w, idx, vort, it, alpha):
    import torch
    nt = mesh.nt
    vin = torch.full((3 * mesh.tcap,), NAN, dtype=torch.float32, device=s.device)
    vin.view(3, mesh.tcap)[:, :nt] = _dev(s, vort.T)
    out = torch.full((3 * mesh.tcap,), NAN, dtype=torch.float32, device=s.device)
    t0, t1 = (torch.full((3 * max(nt, 1),), NAN, dtype=torch.float32, device=s.device) for _ in range(2))
    dw, di = _dev(s, w), _dev(s, idx)
    s.lib.call("mf_vsheet_smooth_iterate", nt, mesh.tcap, _p(dw), _p(di), it, float(f32(alpha)), _p(vin), _p(out), _p(t0), _p(t1), s.stream)
    s.sync()
    return np.ascontiguousarray(out.view(3, mesh.tcap)[:, :nt].cpu().numpy().T)


@pytest.mark.parametrize("name", sorted(set(M.MESHES) - {"empty"}) + sorted(M.OPEN_MESHES))
def test_smoothing(hip_backend, name):
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    is_open = name in M.OPEN_MESHES
    model = (M.OPEN_MESHES if is_open else M.MESHES)[name]()
    nt = model["tris"].shape[0]
    opp = MO.corners(model["tris"])[0]
    st = M.sheet_state(name, nt)
    s = _solver(m)
    _poison_pool(s)
    live = s._live
    mesh = _sheet(m, s, model)
    if not is_open:
        assert np.array_equal(mesh.corners_numpy(), opp)
    differing = 0
    for sigma in M.SMOOTH_SIGMAS:
        key = "smooth/%s/%g" % (name, sigma)
        w_ref, idx_ref = G[key + "/weights"], G[key + "/index"]
        w, idx = _weights_entry(s, mesh, opp, sigma)
        wm, im = M.smooth_weights(model, opp, sigma)
        assert np.array_equal(idx, idx_ref) and np.array_equal(idx, im)
        assert M.ulps_apart(w, w_ref).max() <= M.WEIGHT_ULPS                          # against the reference's float exp
        d = M.ulps_apart(w, wm)
        assert d.max() <= 1 and (d != 0).sum() <= 1, (sigma, int((d != 0).sum()))      # against the host's fp64 exp: the condition
        differing += int((d != 0).sum())
        for it in M.SMOOTH_ITERS:
            want = G["%s/out%d" % (key, it)]
            _same("%s/out%d from the recorded table" % (key, it), _iterate_entry(s, mesh, w_ref, idx_ref, st["vorticity"], it, M.ALPHA), want)
            if is_open:
                continue           # the package refuses a mesh with boundary edges, as the reference's rebuildCorners does
            mesh.set_sheet_numpy(**st)
            vs.smoothVorticity(mesh, iter=it, sigma=sigma, alpha=M.ALPHA)
            got = mesh.sheet_numpy()
            _same("the package's passes are the entry's from its own table", got["vorticitySmoothed"], M.smooth_iterate(w, idx, st["vorticity"], it, M.ALPHA)[1])
            _same("vorticity is read only", got["vorticity"], st["vorticity"])
    print("%s: %d of %d weights differ from the model's" % (name, differing, 2 * 3 * nt))
    if is_open:
        with pytest.raises(RuntimeError, match="can't rebuild corners, index without an opposite"):
            vs.smoothVorticity(mesh)
    assert s._live == live


def test_smoothing_an_empty_sheet_and_iter_zero(hip_backend):
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    s = _solver(m)
    mesh = _sheet(m, s, M.MESHES["empty"]())
    vs.smoothVorticity(mesh, iter=3)
    assert mesh.sheet_numpy()["vorticitySmoothed"].shape == (0, 3)


def test_texcoord_inflow_calls_in_a_row(hip_backend):
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    vs.resetVortexSheetState()
    s = _solver(m)
    _poison_pool(s)
    model = M.MESHES[M.INFLOW_MESH]()
    mesh = _sheet(m, s, model)
    for q, shape in enumerate(M.INFLOW_CALLS):
        vel = _mac(m, s, M.mac_grid("inflow%d" % q))
        live = s._live
        vs.texcoordInflow(mesh, _shape(m, s, shape), vel)
        assert s._live == live                           # the marks, the list and the scan's workspace went back to the pool
        t0 = np.array(vs._state.t0, f32)
        _same("t0", t0, G["inflow/%d/t0" % q])
        _same("mTexOffset", np.array(mesh.getTexOffset(), f32), t0)
        tex1, tex2 = mesh.tex_numpy()
        _same("tex1", tex1, G["inflow/%d/tex1" % q])
        _same("tex2", tex2, G["inflow/%d/tex2" % q])
        if q == 1:
            mesh.reinitTexCoords()
            tex1, tex2 = mesh.tex_numpy()
            _same("reinit", tex1, G["inflow/reinit"])
            _same("reinit", tex2, G["inflow/reinit"])
    assert np.isnan(vs._state.t0).all()                  # the shape of the last call contains no cell
    vs.resetVortexSheetState()
    assert vs._state.t0 == (0.0, 0.0, 0.0)
    # the precondition: a shape with a cell of the last z plane is refused, everything as it was
    before = (mesh.tex_numpy(), mesh.getTexOffset())
    with pytest.raises(RuntimeError, match="^texcoordInflow: the shape contains cells of the last z plane"):
        vs.texcoordInflow(mesh, _shape(m, s, ("box", (2, 2, 2), (6, 6, 16))), _mac(m, s, M.mac_grid("inflow0")))
    after = (mesh.tex_numpy(), mesh.getTexOffset())
    assert before[1] == after[1] and vs._state.t0 == (0.0, 0.0, 0.0)
    _same("tex1", before[0][0], after[0][0])
    other = _solver(m, (9, 8, 7)).create(m.MACGrid)
    with pytest.raises(RuntimeError, match="^texcoordInflow: the velocity grid must be of the mesh's solver's size and device$"):
        vs.texcoordInflow(mesh, _shape(m, s, M.INFLOW_CALLS[0]), other)
    assert vs._state.t0 == (0.0, 0.0, 0.0)
    # after the reset the offset starts from zero again
    vs.texcoordInflow(mesh, _shape(m, s, M.INFLOW_CALLS[0]), _mac(m, s, M.mac_grid("inflow0")))
    _same("t0 from zero again", np.array(vs._state.t0, f32), G["inflow/0/t0"])
    vs.resetVortexSheetState()


@pytest.mark.parametrize("dims", [(7, 6, 5), (33, 31, 29)])
def test_texcoord_inflow_equals_the_model_on_other_grids(hip_backend, dims):
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    vs.resetVortexSheetState()
    s = _solver(m, dims)
    model = MO.bipyramid(32, centre=(3.0, 3.0, 2.0))
    mesh = _sheet(m, s, model)
    n = model["pos"].shape[0]
    t0, tex1, tex2 = np.zeros(3, f32), np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    shapes = (("box", (0.0, 0.0, 0.0), (dims[0], dims[1], dims[2] - 1.25)), ("sphere", (3.2, 3.1, 2.2), 1.9), ("box", (1.0, 0.0, 1.0), (4.0, dims[1], 3.0)))
    for q, shape in enumerate(shapes):
        vel = M.mac_grid("inflow-dims%d" % q, dims)
        vs.texcoordInflow(mesh, _shape(m, s, shape), _mac(m, s, vel))
        t0, tex1, tex2 = M.texcoord_inflow(dims, vel, shape, M.DT, t0, model["pos"], tex1, tex2)
        _same("t0", np.array(vs._state.t0, f32), t0)
        got = mesh.tex_numpy()
        _same("tex1", got[0], tex1)
        _same("tex2", got[1], tex2)
    vs.resetVortexSheetState()


def test_recorded_loop_stage_by_stage_and_at_its_end(hip_backend):
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    C = M.LOOP
    model, flags = M.loop_inputs()
    s = _solver(m, C["dims"], C["dt"])
    _poison_pool(s)
    mesh = _sheet(m, s, model)
    fl = _flag_grid(m, s, flags)
    vvel, vvort = _nan_grid(m, s, m.MACGrid), _nan_grid(m, s, m.VecGrid)
    smoke, g = _shape(m, s, C["smoke"]), m.vec3(*C["gravity"])
    for step in range(C["steps"]):
        vel, old = (_mac(m, s, v) for v in M.loop_velocities(step))
        vs.meshSmokeInflow(mesh, smoke, C["amount"])
        vs.vorticitySource(mesh, g, vel, old, scale=C["scale"], maxAmount=C["maxAmount"], mult=C["mult"])
        got = mesh.sheet_numpy()
        _same("loop/%d/smokeAmount" % step, got["smokeAmount"], G["loop/%d/smokeAmount" % step])
        _same("loop/%d/vorticity" % step, got["vorticity"], G["loop/%d/vorticity" % step])
        # the smoothing is fed the reference's table of this step: a last-bit difference of a weight stays out of the comparison
        w_ref = G["loop/%d/weights" % step]
        opp = mesh.corners_numpy()
        w, idx = _weights_entry(s, mesh, opp, C["sigma"])
        assert M.ulps_apart(w, w_ref).max() <= M.WEIGHT_ULPS
        _same("loop/%d/vorticitySmoothed" % step, _iterate_entry(s, mesh, w_ref, idx, got["vorticity"], C["iters"], C["alpha"]),
              G["loop/%d/vorticitySmoothed" % step])
        vs.smoothVorticity(mesh, iter=C["iters"], sigma=C["sigma"], alpha=C["alpha"])
        sm = mesh.sheet_numpy()["vorticitySmoothed"]
        diff = np.abs(sm.astype(np.float64) - G["loop/%d/vorticitySmoothed" % step]).max()
        print("loop step %d: the package's vorticitySmoothed is within %.3g of the reference's (%d weights differ)"
              % (step, diff, int((w != w_ref).sum())))
        # VICintegration: the spreading within its bound of the reference's; the solve, fed the reference's vort, to the bit
        vs.VICintegration(mesh, C["vic_sigma"], vvel, fl, vorticity=vvort, scale=C["vic_scale"], precondition=2)
        mvort, _, vbound = M.spread(dict(model, pos=mesh.nodes_numpy()[0]), got["vorticity"], flags, C["dims"], C["vic_sigma"], want_bound=True)
        gvort = _planes(vvort)
        assert (np.abs(gvort.T.astype(np.float64) - G["loop/%d/vic_vort" % step].T).max(1) <= vbound).all()
        end_to_end = np.abs(_planes(vvel).astype(np.float64) - G["loop/%d/vic_vel" % step]).max()
        vvort.data.copy_(_dev(s, G["loop/%d/vic_vort" % step].reshape(-1)))
        stats = vs._vic_solve(s.lib, s, vvort, vvel, fl, 1.5, float(f32(1e-3)), float(f32(C["vic_scale"])))
        assert [c["iterations"] for c in stats] == G["loop/%d/vic_iterations" % step].tolist()
        _same("loop/%d/vic_vel" % step, _planes(vvel), G["loop/%d/vic_vel" % step])
        print("loop step %d: VICintegration end to end within %.3g of the reference's velocity (%d vort entries differ)"
              % (step, end_to_end, int((gvort != G["loop/%d/vic_vort" % step]).any(0).sum())))
        mesh.advectInGrid(fl, vvel, 2)
        mesh.reinitTexCoords()
        _same("loop/%d/pos" % step, mesh.nodes_numpy()[0], G["loop/%d/pos" % step])
        tex1, tex2 = mesh.tex_numpy()
        _same("loop/%d/tex1" % step, tex1, G["loop/%d/tex1" % step])
        _same("loop/%d/tex2" % step, tex2, G["loop/%d/tex1" % step])


def test_rebuilding_routes_the_mismatch_and_the_late_refusals(hip_backend, tmp_path):
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    s = _solver(m, (24, 24, 24))
    model = MO.bipyramid(40, centre=(8.0, 8.0, 8.0))
    mesh = _sheet(m, s, model)
    path = str(tmp_path / "sheet.bobj.gz")
    mesh.save(path)
    phi = s.create(m.LevelsetGrid)
    import torch
    phi.data.copy_(torch.from_numpy(MO.two_blobs(24).reshape(-1)).to(phi.data.device))

    def dirty():
        nt, nn = mesh.numTris(), mesh.numNodes()
        mesh.set_sheet_numpy(np.full((nt, 3), 3.0), np.full((nt, 3), 4.0), np.full((nt, 3), 5.0), np.full(nt, 6.0), np.full(nt, 7.0))
        mesh.set_tex_numpy(np.full((nn, 3), 8.0), np.full((nn, 3), 9.0))

    def defaults(nt, nn):
        assert (mesh.numTris(), mesh.numNodes()) == (nt, nn)
        got, want = mesh.sheet_numpy(), M.default_sheet(nt)
        for k in M.DEFAULTS:
            _same(k, got[k], want[k])
        t1, t2 = mesh.tex_numpy()
        k_, e_ = mesh.turb_numpy()
        assert t1.shape == (nn, 3) and not t1.any() and not t2.any() and k_.shape == (nn,) and not k_.any() and not e_.any()

    dirty()
    mesh.set_numpy(model["pos"], None, model["flags"], model["tris"], None)
    defaults(80, 42)
    dirty()
    mesh.load(path)
    defaults(80, 42)
    dirty()
    mesh.clear()
    defaults(0, 0)
    phi.createMesh(mesh)
    nt, nn = mesh.numTris(), mesh.numNodes()
    assert nt > 300
    defaults(nt, nn)
    dirty()
    phi.createMesh(mesh)
    defaults(nt, nn)
    # a route that does not know the channels
    dirty()
    m.killSmallComponents(mesh, 10)
    assert 0 < mesh.numTris() < nt
    before = (mesh.nodes_numpy()[0].tobytes(), mesh.tris_numpy()[0].tobytes())
    box = _shape(m, s, ("box", (1, 1, 1), (9, 9, 9)))
    vel = s.create(m.MACGrid)
    msg = r"channels do not match the mesh \(%d triangles and %d nodes, channels of %d and %d\)" % (mesh.numTris(), mesh.numNodes(), nt, nn)
    for who, call in (("calcVorticity", mesh.calcVorticity), ("reinitTexCoords", mesh.reinitTexCoords), ("sheet_numpy", mesh.sheet_numpy),
                      ("meshSmokeInflow", lambda: vs.meshSmokeInflow(mesh, box, 1.0)), ("vorticitySource", lambda: vs.vorticitySource(mesh, m.vec3(0, -1, 0))),
                      ("smoothVorticity", lambda: vs.smoothVorticity(mesh)), ("texcoordInflow", lambda: vs.texcoordInflow(mesh, box, vel))):
        with pytest.raises(RuntimeError, match="^VortexSheetMesh::%s: %s$" % (who, msg)):
            call()
    assert (mesh.nodes_numpy()[0].tobytes(), mesh.tris_numpy()[0].tobytes()) == before and vs._state.t0 == (0.0, 0.0, 0.0)
    # the argument checks come after the refusals by name
    mesh.load(path)
    plain = s.create(m.Mesh)
    for call in (lambda: vs.meshSmokeInflow(plain, box, 1.0), lambda: vs.smoothVorticity(plain), lambda: vs.vorticitySource(plain, m.vec3(0, 0, 0))):
        with pytest.raises(RuntimeError, match=r"^can't convert argument to VortexSheetMesh\*$"):
            call()
    with pytest.raises(RuntimeError, match=r"^can't convert argument to Shape\*$"):
        vs.meshSmokeInflow(mesh, vel, 1.0)
    with pytest.raises(RuntimeError, match=r"^can't convert argument to MACGrid\*$"):
        vs.texcoordInflow(mesh, box, phi)
    with pytest.raises(RuntimeError, match="argument is not an int"):
        vs.smoothVorticity(mesh, iter=1.5)
    with pytest.raises(RuntimeError, match="Argument .* unknown"):
        vs.smoothVorticity(mesh, sigm=0.2)
    # a 2-D solver, after the z-slab and backend refusals
    s2 = _solver(m, (12, 12, 1), dim=2)
    flat = s2.create(vs.VortexSheetMesh)
    for who, call in (("VortexSheetMesh::calcVorticity", flat.calcVorticity), ("meshSmokeInflow", lambda: vs.meshSmokeInflow(flat, box, 1.0)),
                      ("smoothVorticity", lambda: vs.smoothVorticity(flat))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == who + ": 3-D solvers only"
    s2._slab_window = (2, 8)
    with pytest.raises(RuntimeError) as e:
        vs.smoothVorticity(flat)
    assert str(e.value) == "smoothVorticity: vortex sheets do not run on a z-slab solver"


# ---- VICintegration ---------------------------------------------------------------------------------------------------------------------
def _flag_grid(m, s, flags):
    import torch
    g = s.create(m.FlagGrid)
    g.data.copy_(torch.from_numpy(flags).to(g.data.device))
    return g


def _nan_grid(m, s, cls):
    g = s.create(cls)
    g.data.fill_(NAN)
    return g


def _planes(g):
    return g.data.cpu().numpy().reshape(3, -1).copy()


@pytest.mark.parametrize("name", sorted(M.vic_cases()))
def test_vic_spreading(hip_backend, name):
    """the spreading through the plugin: HIP = model bit for bit but for the cells of at most one triangle's stencil (a weight whose
    fp64 cos the device rounds the other way), and HIP within the derived bound of the reference; outputs and scratch pre-filled with NaN"""
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    dims, sigma, T, rev = M.vic_cases()[name]
    model_mesh, vorticity = M.vic_soup(dims, T, 1, rev)
    flags = M.vic_flags(dims)
    s = _solver(m, dims)
    _poison_pool(s, 14)
    mesh = _sheet(m, s, model_mesh)
    mesh.set_sheet_numpy(vorticity=vorticity)
    live = s._live
    vel, vort = _nan_grid(m, s, m.MACGrid), _nan_grid(m, s, m.VecGrid)
    vs.VICintegration(mesh, sigma, vel, _flag_grid(m, s, flags), vorticity=vort, cgMaxIterFac=0.3, precondition=2)
    got = np.ascontiguousarray(_planes(vort).T)
    want, wnorm, bound = M.spread(model_mesh, vorticity, flags, dims, sigma, want_bound=True)
    ref = np.ascontiguousarray(G["vic/%s/vort" % name].T)
    assert not np.isnan(got).any() and not np.isnan(_planes(vel)).any()
    assert not got[bound == 0].any()                                        # where nothing lands the entry is exactly 0
    err = np.abs(got.astype(np.float64) - ref).max(1)
    assert (err <= bound).all()
    hit = bound > 0
    differs = np.nonzero((got != want).any(1))[0]
    print("%s: largest error %.3g of the bound; %d of %d entries not bit-identical to the reference, %d to the model"
          % (name, float((err[hit] / bound[hit]).max()) if hit.any() else 0.0, int((got != ref).any(1).sum()), int(hit.sum()), differs.size))
    if differs.size:                                                        # the condition: one triangle's stencil at the most
        sgi = int(np.ceil(sigma))
        ijk = np.stack([differs % dims[0], (differs // dims[0]) % dims[1], differs // (dims[0] * dims[1])], 1)
        assert ((ijk.max(0) - ijk.min(0)) < 2 * sgi).all()
        assert (np.abs(got.astype(np.float64) - want).max(1) <= bound).all()
    st = vs.lastVortexSheetStats()["vic"]
    assert len(st) == 3 and all(set(c) == {"iterations", "residual"} for c in st)
    del vel, vort
    assert s._live == live                                                  # every grid of the call went back to the pool


@pytest.mark.parametrize("name", M.VIC_SOLVES)
@pytest.mark.parametrize("kind", ["mac", "vec3"])
def test_vic_solve_from_the_recorded_vorticity(hip_backend, name, kind):
    """curl, right-hand sides, the three CG solves and the scaled components from the reference's own vort: bit for bit, iteration counts
    included"""
    import torch
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    dims = M.vic_cases()[name][0]
    s = _solver(m, dims)
    _poison_pool(s, 14)
    vort = s.create(m.VecGrid)
    vort.data.copy_(torch.from_numpy(G["vic/%s/vort" % name].reshape(-1)).to(vort.data.device))
    vel = _nan_grid(m, s, m.MACGrid if kind == "mac" else m.VecGrid)
    flags = _flag_grid(m, s, M.vic_flags(dims))
    C = M.VIC_SOLVE
    vs._vic_keep = keep = []
    try:
        stats = vs._vic_solve(s.lib, s, vort, vel, flags, float(f32(C["cgMaxIterFac"])), float(f32(C["cgAccuracy"])), float(f32(C["scale"])))
    finally:
        vs._vic_keep = None
    key = "vic/%s/%s" % (name, kind)
    assert [c["iterations"] for c in stats] == G[key + "/iterations"].tolist()
    if key + "/rhs" in G:
        _same("rhs", np.stack(keep), G[key + "/rhs"])
    _same("vel", _planes(vel), G[key + "/vel"])
    _same("vort is read only", _planes(vort), G["vic/%s/vort" % name])


def test_vic_refusals(hip_backend):
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    dims = M.VIC_GRIDS[0]
    s = _solver(m, dims)
    mesh = _sheet(m, s, M.vic_soup(dims, 5, 1)[0])
    vel, flags = _nan_grid(m, s, m.MACGrid), _flag_grid(m, s, M.vic_flags(dims))
    for bad in (0, 3):
        with pytest.raises(RuntimeError) as e:
            vs.VICintegration(mesh, 1.5, vel, flags, precondition=bad)
        assert str(e.value) == bytes(G["vic/precondition%d" % bad]).decode() == "GridCg<APPLYMAT>::setICPreconditioner: Invalid method specified."
    with pytest.raises(RuntimeError) as e:
        vs.VICintegration(mesh, 1.5, vel, flags)                           # the reference's own default fails as well
    assert "setICPreconditioner" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        vs.VICintegration(mesh, 1.5, vel, flags, precondition=1)
    assert str(e.value) == "VICintegration: the plain incomplete-Cholesky preconditioner (precondition=1) is not implemented"
    with pytest.raises(RuntimeError, match=r"^can't convert argument to FlagGrid$"):
        vs.VICintegration(mesh, 1.5, vel, vel, precondition=2)
    with pytest.raises(RuntimeError, match=r"^can't convert argument to VortexSheetMesh\*$"):
        vs.VICintegration(s.create(m.Mesh), 1.5, vel, flags, precondition=2)
    assert np.isnan(_planes(vel)).all()
    s2 = _solver(m, (12, 12, 1), dim=2)
    with pytest.raises(RuntimeError) as e:
        vs.VICintegration(s2.create(vs.VortexSheetMesh), 1.5, vel, flags, precondition=2)
    assert str(e.value) == "VICintegration: 3-D solvers only"
