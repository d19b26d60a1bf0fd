"""GPU: the smoke data-generation plugins (include/open/manta_hip_datagen.h) against the numpy statement of tests/datagen_model.py
and the reference's recorded outputs (tests/golden/datagen.npz): blur, projection and Laplacian bit for bit, curvature within one fp32
ulp of the reference value in every cell (the device's fp64 pow need not round like the C library's), the centre of mass bit for bit
against the contract and within the derived bound of the reference's serial fp32 sum.  Outputs and pool scratch are pre-filled with
NaN."""
import ctypes

import numpy as np
import pytest

import datagen_model as M

pytestmark = pytest.mark.gpu

GOLDEN = np.load(M.GOLDEN)
f32 = np.float32


def solver(m, dims):
    return m.Solver(name="s", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)


def poison_pool(s, kind, count=2):
    """`count` NaN-filled tensors on top of the solver's pool: what the next scratch grids of that kind will be"""
    ts = [s._alloc(kind, zero=False) for _ in range(count)]
    for t in ts:
        t.fill_(float("nan"))
        s._release(kind, t)


def grid_from(s, cls, a):
    g = s.create(cls)
    g.from_numpy(a)
    return g


def poisoned(s, cls):
    g = s.create(cls)
    g.data.fill_(float("nan"))
    return g


def same(tag, got, want):
    assert M.same(got, want), "%s: %d of %d elements differ" % (tag, M.differing(np.asarray(got), np.asarray(want)), np.asarray(want).size)


# ---- weights ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,mdim", M.WEIGHT_SIGMAS)
def test_weights(hip_backend, sigma, mdim):
    from mantaflow_amd import _lib
    lib = _lib.get()
    w = np.full(M.MAX_TAPS, np.nan, f32)
    n = ctypes.c_int(-1)
    lib.call("mf_datagen_weights", float(f32(sigma)), w.size, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n))
    wn, ww = M.weights(sigma)
    assert n.value == wn == mdim
    same("weights", w[:wn], ww)
    assert np.isnan(w[wn:]).all()
    with pytest.raises(RuntimeError, match="more than 3 taps"):
        lib.call("mf_datagen_weights", 1.128, 3, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n))
    with pytest.raises(RuntimeError, match="sigma must be positive"):
        lib.call("mf_datagen_weights", 0.0, w.size, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n))


# ---- blur -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dims,sigma", M.blur_cases(), ids=[c[0] for c in M.blur_cases()])
def test_blur(hip_backend, name, dims, sigma):
    import manta as m
    s = solver(m, dims)
    for ncomp, key, cls, plug, kind in ((1, "real", m.RealGrid, m.blurRealGrid, "real"), (3, "mac", m.MACGrid, m.blurMacGrid, "vec")):
        src = M.blur_input(name, ncomp)
        want = GOLDEN["blur/%s/%s" % (name, key)]
        same("the model", M.blur(src, sigma)[0], want)
        oG, tG = grid_from(s, cls, src), poisoned(s, cls)
        poison_pool(s, kind)
        live, pooled = s._live, len(s._pool[kind])
        assert plug(oG, tG, sigma) == int(GOLDEN["blur/%s/mdim" % name][0])
        same("%s tG" % key, tG.to_numpy(), want)
        same("%s oG" % key, oG.to_numpy(), src)                       # oG is never written unless it is tG
        assert (s._live, len(s._pool[kind])) == (live, pooled)        # scratch is back in the pool
        # a second call in a row reuses the scratch, which now holds the first call's intermediates
        tG.data.fill_(float("nan"))
        plug(oG, tG, sigma)
        same("%s tG, second call" % key, tG.to_numpy(), want)
        assert (s._live, len(s._pool[kind])) == (live, pooled)
        # oG is tG
        poison_pool(s, kind)
        assert plug(oG, oG, si=sigma) == int(GOLDEN["blur/%s/mdim" % name][0])
        same("%s oG is tG" % key, oG.to_numpy(), want)


def test_blur_refuses_a_sigma_that_is_not_positive(hip_backend):
    import manta as m
    s = solver(m, (9, 7, 5))
    src = M.blur_input("special", 1)
    oG, tG = grid_from(s, m.RealGrid, src), grid_from(s, m.RealGrid, src * f32(2))
    live = s._live
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="^blurRealGrid: sigma must be positive$"):
            m.blurRealGrid(oG, tG, bad)
    with pytest.raises(RuntimeError, match="more than 255 taps"):
        m.blurRealGrid(oG, tG, 50.0)
    same("oG", oG.to_numpy(), src)
    same("tG", tG.to_numpy(), src * f32(2))
    assert s._live == live


# ---- centre of mass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.COM_CASES)
def test_center_of_mass(hip_backend, name):
    import manta as m
    d = M.com_input(name)
    s = solver(m, M.dims_of(d))
    c = m.calcCenterOfMass(grid_from(s, m.RealGrid, d))
    got = np.array([c.x, c.y, c.z], f32)
    assert (got.astype(np.float64) == [c.x, c.y, c.z]).all()
    ref = GOLDEN["com/%s" % name]
    same("against the contract", got, M.center_of_mass(d))
    if name in M.COM_EXACT:
        same("against the reference", got, ref)
    else:
        bound = M.com_bound(d, ref)
        for q in range(3):
            err = abs(float(got[q]) - float(ref[q]))
            print(name, "xyz"[q], "HIP - reference", err, "bound", bound[q])
            assert err <= bound[q]
    c2 = m.calcCenterOfMass(grid_from(s, m.RealGrid, d))                # the same bits on every run
    same("second run", np.array([c2.x, c2.y, c2.z], f32), got)


# ---- projection -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", M.PROJECT_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_projection(hip_backend, tmp_path, dims):
    import manta as m
    s = solver(m, dims)
    val = grid_from(s, m.RealGrid, M.project_input(dims))
    for mode in M.PROJECT_MODES:
        for scale in M.PROJECT_SCALES:
            want = GOLDEN[M.project_key(dims, mode, scale)]
            img = m.projectImage(val, mode, scale)
            assert img.dtype == np.uint8
            same("projectImage mode %d scale %g" % (mode, scale), img, want)
            path = str(tmp_path / ("m%d_s%g.ppm" % (mode, scale)))
            m.projectPpmFull(val, path, mode, scale)
            assert open(path, "rb").read() == M.ppm_bytes(want), (mode, scale)
    same("the defaults", m.projectImage(val), GOLDEN[M.project_key(dims, 0, 1.0)])
    same("val", val.to_numpy(), M.project_input(dims))


def test_projection_of_a_constant_grid_and_the_file_error(hip_backend, tmp_path):
    import manta as m
    s = solver(m, (7, 5, 4))
    val = grid_from(s, m.LevelsetGrid, M.project_const())
    same("constant grid, surfaces", m.projectImage(val, shadeMode=1), GOLDEN["project/const"])
    bad = str(tmp_path / "no_such_dir" / "x.ppm")
    with pytest.raises(RuntimeError) as err:
        m.projectPpmFull(val, bad, 1, 1.0)
    assert "projectPpmFull" in str(err.value) and bad in str(err.value)
    thin = solver(m, (7, 5, 2))
    with pytest.raises(RuntimeError, match="thinner than 3 cells"):
        m.projectImage(thin.create(m.RealGrid), 1)
    assert m.projectImage(thin.create(m.RealGrid), 0).shape == (7, 16, 3)


# ---- Laplacian and curvature --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,kind,dims,h", M.stencil_cases(), ids=[c[0] for c in M.stencil_cases()])
def test_laplacian_and_curvature(hip_backend, key, kind, dims, h):
    import manta as m
    s = solver(m, dims)
    g = M.stencil_input(kind, dims)
    grid = grid_from(s, m.LevelsetGrid if kind == "sphere" else m.RealGrid, g)
    out = grid_from(s, m.RealGrid, np.full(g.shape, M.SENTINEL, f32))
    want = GOLDEN[key]
    border = np.ones(g.shape, bool)
    border[M._inner(g)] = False
    if h is None:
        m.getLaplacian(out, grid)
        got = out.to_numpy()
        same(key, got, want)
    else:
        if h == 1.0:
            m.getCurvature(out, grid)
        else:
            m.getCurvature(out, grid, h)
        got = out.to_numpy()
        ok, nd = M.within_one_ulp(got, want)
        print("%s: %d of %d cells are not bit-identical to the reference" % (key, nd, int((~border).sum())))
        assert ok, key                                               # 1 fp32 ulp of the reference value, no cell exempt
    assert (got[border] == M.SENTINEL).all()
    same("grid", grid.to_numpy(), g)


def test_stencil_outputs_may_not_alias(hip_backend):
    import manta as m
    s = solver(m, (7, 5, 4))
    g = M.stencil_input("noise", (7, 5, 4))
    grid = grid_from(s, m.RealGrid, g)
    with pytest.raises(ValueError, match="^getLaplacian: the output grid must not be the input grid$"):
        m.getLaplacian(grid, grid)
    with pytest.raises(ValueError, match="^getCurvature: the output grid must not be the input grid$"):
        m.getCurvature(grid, grid, 0.5)
    same("grid", grid.to_numpy(), g)


# ---- the two loops against recorded reference runs ----------------------------------------------------------------------------------
def mac_planes(g):
    """a MACGrid as the recorded [3][z][y][x]"""
    return np.ascontiguousarray(np.moveaxis(g.to_numpy(), -1, 0))


def test_surface_tension_loop(hip_backend):
    """scenes/surfaceTension.py at 20^3 for 5 steps, without the mesh line"""
    import manta as m
    vec3 = m.vec3
    C = M.ST_LOOP
    res = C["res"]
    gs = vec3(res, res, res)
    s = m.Solver(name="main", gridSize=gs, dim=3)
    s.timestep = 0.25
    curv, flags, vel, pressure = s.create(m.RealGrid), s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.RealGrid)
    flags.initDomain(boundaryWidth=1)
    fluidbox = m.Box(parent=s, p0=gs * vec3(0.25, 0.25, 0.25), p1=gs * vec3(0.75, 0.75, 0.75))
    phi = fluidbox.computeLevelset()
    flags.updateFromLevelset(phi)
    its = []
    for t in range(C["steps"]):
        phi.reinitMarching(flags=flags, velTransport=vel)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=phi, order=1)
        phi.setBoundNeumann(1)
        flags.updateFromLevelset(phi)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2)
        m.setWallBcs(flags=flags, vel=vel)
        m.getCurvature(curv=curv, grid=phi)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure, phi=phi, curv=curv, surfTens=0.1, cgAccuracy=5e-4)
        its.append(m.lastCgStats()["iterations"])
        s.step()
    assert its == list(GOLDEN["st/iterations"])
    ok, nd = M.within_one_ulp(curv.to_numpy(), GOLDEN["st/curv"])
    print("surface tension loop: %d of %d cells of curv are not bit-identical to the reference" % (nd, res ** 3))
    assert ok
    if nd == 0:
        same("phi", phi.to_numpy(), GOLDEN["st/phi"])
        same("vel", mac_planes(vel), GOLDEN["st/vel"])
    else:       # a curvature one ulp off feeds the solve: the package's relative parity bound for fp32 fields
        for tag, got, want in (("phi", phi.to_numpy(), GOLDEN["st/phi"]), ("vel", mac_planes(vel), GOLDEN["st/vel"])):
            err = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
            print("surface tension loop: %s relative error %.3g" % (tag, err))
            assert err <= 1e-5, tag


def test_data_generation_loop(hip_backend):
    """the simMode == 1 loop of manta_genSimData2.py: fine grid 32^3, coarse grid 16^3, re-centring on, the constants of DG_LOOP"""
    import manta as m
    vec3 = m.vec3
    C = M.DG_LOOP
    res, scaleFactor, resetN, bWidth = C["res"], C["scaleFactor"], C["resetN"], 1
    sm_gs = vec3(res, res, res)
    xl_gs = vec3(res * scaleFactor, res * scaleFactor, res * scaleFactor)
    sm = m.Solver(name="smaller", gridSize=sm_gs, dim=3)
    xl = m.Solver(name="larger", gridSize=xl_gs, dim=3)
    flags, vel, density, tmp = sm.create(m.FlagGrid), sm.create(m.MACGrid), sm.create(m.RealGrid), sm.create(m.RealGrid)
    xl_flags, xl_vel, xl_density = xl.create(m.FlagGrid), xl.create(m.MACGrid), xl.create(m.RealGrid)
    xl_velTmp, xl_tmp = xl.create(m.MACGrid), xl.create(m.RealGrid)
    velRecenter, xl_velRecenter = sm.create(m.MACGrid), xl.create(m.MACGrid)
    for f in (flags, xl_flags):
        f.initDomain(boundaryWidth=bWidth)
        f.fillGrid()
        m.setOpenBound(f, bWidth, "yY", m.FlagOutflow | m.FlagEmpty)
    noise, noiSm, sources, sourSm = [], [], [], []
    for q in range(2):
        c, (r_xl, r_sm), (posScale, valOffset, timeAnim) = C["src"][q], C["srcr"][q], C["noise"][q]
        for lst, solver, anim in ((noise, xl, timeAnim), (noiSm, sm, timeAnim / float(scaleFactor))):
            n = solver.create(m.NoiseField, fixedSeed=C["seeds"][q], loadFromFile=True)
            n.posScale, n.clamp, n.clampNeg, n.clampPos, n.valScale, n.valOffset = vec3(posScale), True, 0, 1.0, 1.0, valOffset
            n.timeAnim, n.posOffset = anim, vec3(1.5)
            lst.append(n)
        sources.append(xl.create(m.Sphere, center=vec3(*c[0:3]), radius=r_xl, scale=vec3(*c[6:9])))
        sourSm.append(sm.create(m.Sphere, center=vec3(*c[3:6]), radius=r_sm, scale=vec3(*c[6:9])))
        m.densityInflow(flags=xl_flags, density=xl_density, noise=noise[q], shape=sources[q], scale=1.0, sigma=1.0)
        m.densityInflow(flags=flags, density=density, noise=noiSm[q], shape=sourSm[q], scale=1.0, sigma=1.0)
    inflowSrc = [1]
    inivel = []
    for c in C["ini"]:
        inivel.append((xl.create(m.Sphere, center=vec3(*c[0:3]), radius=c[3], scale=vec3(1)), vec3(*c[4:7]),
                       sm.create(m.Sphere, center=vec3(*c[7:10]), radius=c[10], scale=vec3(1)), vec3(*c[11:14])))
    buoy, xl_buoy = vec3(0, C["buoy"][0], 0), vec3(0, C["buoy"][1], 0)
    blurSig = float(scaleFactor) / 3.544908
    xl_velTmp.copyFrom(xl_vel)
    assert m.blurMacGrid(xl_vel, xl_velTmp, blurSig) == 5
    m.interpolateMACGrid(target=vel, source=xl_velTmp)
    vel.multConst(vec3(1. / scaleFactor))
    its, centres_differ = [], 0
    for t in range(C["steps"]):
        # calcCOM with re-centring on.  The plugin's fp64 sum may differ from the reference's serial fp32 sum in the last bits, and the
        # centre feeds the advection: the plugin's own value is held to the derived bound and the recorded centre drives the loop, so
        # everything after it must be bit-identical (where the two centres are equal that is the loop exactly as recorded)
        c = m.calcCenterOfMass(xl_density)
        got, ref = np.array([c.x, c.y, c.z], f32), GOLDEN["dg/com"][t]
        d = xl_density.to_numpy()
        same("step %d: the centre against the contract" % t, got, M.center_of_mass(d))
        if not M.same(got, ref):
            centres_differ += 1
            bound = M.com_bound(d, ref)
            for q in range(3):
                err = abs(float(got[q]) - float(ref[q]))
                print("step %d %s: HIP centre - reference %.3g, bound %.3g" % (t, "xyz"[q], err, bound[q]))
                assert err <= bound[q]
        off = f32(0.5) * np.array([xl_gs.x, xl_gs.y, xl_gs.z], f32) - ref        # xl_gs * 0.5 - newCentre, in fp32
        off = off * f32(1. / xl.timestep)
        xl_velOffset = vec3(*[float(v) for v in off])
        velOffset = vec3(*[float(v * f32(1. / float(scaleFactor))) for v in off])
        for nI in inflowSrc:
            m.densityInflow(flags=xl_flags, density=xl_density, noise=noise[nI], shape=sources[nI], scale=1.0, sigma=1.0)
            m.densityInflow(flags=flags, density=density, noise=noiSm[nI], shape=sourSm[nI], scale=1.0, sigma=1.0)
        # high res fluid
        m.advectSemiLagrange(flags=xl_flags, vel=xl_velRecenter, grid=xl_vel, order=2, clampMode=2, openBounds=True, boundaryWidth=bWidth)
        m.setWallBcs(flags=xl_flags, vel=xl_vel)
        m.addBuoyancy(density=xl_density, vel=xl_vel, gravity=buoy, flags=xl_flags)
        for sph, v, _, _ in inivel:
            sph.applyToGrid(grid=xl_vel, value=v)
        if t < C["warm"]:
            m.vorticityConfinement(vel=xl_vel, flags=xl_flags, strength=0.05)
        m.solvePressure(flags=xl_flags, vel=xl_vel, pressure=xl_tmp, cgMaxIterFac=2.0, cgAccuracy=0.001, preconditioner=m.PcMGStatic)
        step_its = [m.lastCgStats()["iterations"], -1]
        m.setWallBcs(flags=xl_flags, vel=xl_vel)
        xl_velRecenter.copyFrom(xl_vel)
        xl_velRecenter.addConst(xl_velOffset)
        m.advectSemiLagrange(flags=xl_flags, vel=xl_velRecenter, grid=xl_density, order=2, clampMode=2, openBounds=True, boundaryWidth=bWidth)
        # low res fluid, velocity
        if t % resetN == 0:
            xl_velTmp.copyFrom(xl_vel)
            m.blurMacGrid(xl_vel, xl_velTmp, blurSig)
            m.interpolateMACGrid(target=vel, source=xl_velTmp)
            vel.multConst(vec3(1. / scaleFactor))
        else:
            m.advectSemiLagrange(flags=flags, vel=velRecenter, grid=vel, order=2, clampMode=2, openBounds=True, boundaryWidth=bWidth)
            m.setWallBcs(flags=flags, vel=vel)
            m.addBuoyancy(density=density, vel=vel, gravity=xl_buoy, flags=flags)
            for _, _, sph, v in inivel:
                sph.applyToGrid(grid=vel, value=v)
            if t < C["warm"]:
                m.vorticityConfinement(vel=vel, flags=flags, strength=0.05 / scaleFactor)
            m.solvePressure(flags=flags, vel=vel, pressure=tmp, cgMaxIterFac=2.0, cgAccuracy=0.001, preconditioner=m.PcMGStatic)
            step_its[1] = m.lastCgStats()["iterations"]
            m.setWallBcs(flags=flags, vel=vel)
        velRecenter.copyFrom(vel)
        velRecenter.addConst(velOffset)
        # low res fluid, density
        if t % resetN == 0:
            xl_tmp.copyFrom(xl_density)
            m.blurRealGrid(xl_density, xl_tmp, blurSig)
            m.interpolateGrid(target=density, source=xl_tmp)
        else:
            m.advectSemiLagrange(flags=flags, vel=velRecenter, grid=density, order=2, clampMode=2, openBounds=True, boundaryWidth=bWidth)
        its.append(step_its)
        sm.step()
        xl.step()
    print("data-generation loop: the plugin's centre differs from the recorded one in %d of %d steps" % (centres_differ, C["steps"]))
    assert its == [list(r) for r in GOLDEN["dg/iterations"]]
    same("fine density", xl_density.to_numpy(), GOLDEN["dg/xl_density"])
    same("coarse density", density.to_numpy(), GOLDEN["dg/density"])
    same("coarse vel", mac_planes(vel), GOLDEN["dg/vel"])
    same("image of the fine density", m.projectImage(xl_density, 0, 5.0), GOLDEN["dg/img_high"])
    same("image of the coarse density", m.projectImage(density, 0, 5.0), GOLDEN["dg/img_low"])
    m.releaseMG(sm)
    m.releaseMG(xl)
