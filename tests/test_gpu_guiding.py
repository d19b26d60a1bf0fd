"""GPU: fluid guiding on the HIP backend (include/manta_hip_guiding.h, PD_fluid_guiding), everything bit for bit:

  * the library's Gaussian weights against the reference's recorded ones (which also says that this machine's C library rounds expf
    as the recording machine's did);
  * the blur and the three fused kernels against the numpy model tests/guiding_model.py, which tests/test_guiding_model.py ties to
    the reference;
  * whole PD_fluid_guiding loops against recorded reference runs (tests/golden/guiding.npz, tools/record_guiding.py): primal-dual
    iterations per step, CG iterations of every inner solve, and the final grids.  These rest on the solvePressure parity the
    other GPU tests assert: if the kernel tests here pass and a loop differs, the difference is in the inner solve."""
import ctypes

import numpy as np
import pytest

import guiding_model as M
from util import assert_bitexact

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def G():
    return M.golden()


@pytest.fixture
def lib(hip_backend):
    import manta as m
    from mantaflow_amd import _lib
    m.releaseBlurPrecomp()
    yield _lib.get()
    m.releaseBlurPrecomp()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def soa(g):
    """[z][y][x][3] -> [3][n]"""
    return np.ascontiguousarray(np.asarray(g, f32).reshape(-1, 3).T)


def aos(t, shape):
    return np.ascontiguousarray(t.cpu().numpy().reshape(3, -1).T.reshape(shape + (3,)))


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def lib_weights(lib, radius):
    w = np.full(2 * radius + 1, np.nan, f32)
    lib.call("mf_guiding_weights", radius, w.ctypes.data_as(ctypes.c_void_p))
    return w


# ---- weights ---------------------------------------------------------------------------------------------------------------------------
def test_weights(lib, G):
    for r in M.RADII:
        assert_bitexact(lib_weights(lib, r), G["weights/%d" % r], "weights of radius %d" % r)
    with pytest.raises(RuntimeError, match="invalid radius"):
        lib.call("mf_guiding_weights", -1, np.zeros(1, f32).ctypes.data_as(ctypes.c_void_p))


# ---- blur ------------------------------------------------------------------------------------------------------------------------------
BLUR_SHAPES = [((37, 5, 3), 2), ((6, 41, 7), 5), ((9, 7, 35), 1), ((8, 8, 8), 0), ((5, 4, 3), 8), ((33, 18, 1), 2), ((3, 50, 1), 5)]


def flag_grids(dims):
    sx, sy, sz = dims
    shape = (sz, sy, sx)
    rng = np.random.RandomState(sx * 10007 + sy * 101 + sz)
    rnd = np.where(rng.uniform(size=shape) < 0.15, M.OBSTACLE, M.FLUID).astype(np.int32)
    # obstacles on the i = 0, j = 0, k = 0 faces (whose lower neighbours do not exist) and on the last planes
    rnd[sz // 2, sy // 2, 0] = rnd[sz // 2, 0, sx // 2] = rnd[0, sy // 2, sx // 2] = M.OBSTACLE
    rnd[sz // 2, sy // 2, sx - 1] = rnd[sz // 2, sy - 1, sx // 2] = rnd[sz - 1, sy // 2, sx // 3] = M.OBSTACLE
    rnd[0, 0, 0] = M.OBSTACLE
    return {"free": np.full(shape, M.FLUID, np.int32), "all obstacle": np.full(shape, M.OBSTACLE, np.int32), "random": rnd}


@pytest.mark.parametrize("dims,radius", BLUR_SHAPES)
def test_blur_equals_model(lib, dims, radius):
    import torch
    sx, sy, sz = dims
    shape, n, is3d = (sz, sy, sx), sx * sy * sz, sz > 1
    w = M.weights(radius)
    assert_bitexact(lib_weights(lib, radius), w, "weights")
    w_dev = dev(w)
    a = np.random.RandomState(radius + n).uniform(-2, 2, shape + (3,)).astype(f32)
    for tag, flags in flag_grids(dims).items():
        fl = dev(flags)
        for times in (1, 2):
            grid = dev(soa(a))
            s1 = torch.full((3 * n,), float("nan"), dtype=torch.float32, device="cuda")
            s2 = torch.full((3 * n,), float("nan"), dtype=torch.float32, device="cuda") if is3d else None
            lib.call("mf_guiding_blur", sx, sy, sz, P(fl), P(grid), P(s1), None if s2 is None else P(s2), P(w_dev), radius, times, None)
            torch.cuda.synchronize()
            want = M.blur(a, flags, w, is3d, times)
            assert np.isfinite(want).all()
            assert_bitexact(aos(grid, shape), want, "blur %s r=%d %s times=%d" % (dims, radius, tag, times))
            if tag == "all obstacle":
                assert_bitexact(want, a, "all cells kept")


def test_blur_refuses_bad_arguments(lib):
    import torch
    t = torch.zeros(3 * 8 * 8 * 8, device="cuda")
    fl = torch.ones(8 * 8 * 8, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="missing grid, scratch or weights"):
        lib.call("mf_guiding_blur", 8, 8, 8, P(fl), P(t), P(t), None, P(t), 1, 1, None)      # a 3-D blur needs the second scratch grid
    with pytest.raises(RuntimeError, match="invalid radius"):
        lib.call("mf_guiding_blur", 8, 8, 8, P(fl), P(t), P(t), P(t), P(t), -1, 1, None)


# ---- fused element-wise kernels ------------------------------------------------------------------------------------------------------
PARAMS = {"scene 2-D": (0.99 / 1.0, 1.0, 1.0), "scene 3-D": (2.44 / (0.58 / 2), 0.58 / 2, 0.3), "thirds": (0.1, 1.0 / 3.0, 0.7)}


@pytest.mark.parametrize("dims", [(7, 5, 3), (33, 31, 29)])
@pytest.mark.parametrize("pname", list(PARAMS))
def test_fused_kernels_equal_model(lib, dims, pname):
    import torch
    sigma, tau, theta = PARAMS[pname]
    sx, sy, sz = dims
    shape, n = (sz, sy, sx), sx * sy * sz
    rng = np.random.RandomState(n)
    g = lambda: rng.uniform(-1.5, 1.5, shape + (3,)).astype(f32)
    x, y, Q, velC, z, vnb = g(), g(), g(), g(), g(), g()
    weight = rng.uniform(-0.2, 2.0, shape).astype(f32)
    weight.ravel()[::7] = 0
    sig = f32(sigma)
    # precomputeInvA, with sigma as it is and with a negative one that takes the clamp at 0.01
    for sg in (sig, f32(-0.5)):
        inv, w_d = torch.full((n,), float("nan"), device="cuda"), dev(weight)
        lib.call("mf_guiding_inv_a", n, P(w_d), float(sg), P(inv), None)
        assert_bitexact(inv.cpu().numpy().reshape(shape), M.inv_a(weight, sg), "invA sigma=%r" % sg)
    invA = M.inv_a(weight, sig)
    assert (M.inv_a(weight, f32(-0.5)) == f32(1.0 / float(f32(0.01)))).any()
    # pre
    xv_d, vn_d = (torch.full((3 * n,), float("nan"), device="cuda") for _ in range(2))
    x_d, y_d, Q_d, invA_d, vnb_d, velC_d = dev(soa(x)), dev(soa(y)), dev(soa(Q)), dev(invA), dev(soa(vnb)), dev(soa(velC))    # kept alive
    lib.call("mf_guiding_pre", n, P(x_d), P(y_d), P(Q_d), P(invA_d), P(xv_d), P(vn_d), float(f32(1.0 / float(sig))), float(sig), None)
    xv, vn = M.pre(x, y, Q, invA, sigma)
    assert_bitexact(aos(xv_d, shape), xv, "xv")
    assert_bitexact(aos(vn_d, shape), vn, "vn")
    assert_bitexact(aos(x_d, shape), x, "x is left alone by the first kernel")
    # mid, on a seeded stand-in for the blurred grid
    zn_d = torch.full((3 * n,), float("nan"), device="cuda")
    z_d = dev(soa(z))
    lib.call("mf_guiding_mid", n, P(x_d), P(y_d), P(xv_d), P(vnb_d), P(invA_d), P(velC_d), P(z_d), P(zn_d), float(sig),
             float(f32(tau)), None)
    x1, z1 = M.mid(x, y, xv, vnb, invA, velC, z, sigma, tau)
    assert_bitexact(aos(x_d, shape), x1, "x")
    assert_bitexact(aos(zn_d, shape), z1, "z before the solve")
    assert_bitexact(aos(z_d, shape), z, "the old z stays: it is z0")
    # post
    out = (ctypes.c_float * 2)()
    lib.call("mf_guiding_post", n, P(zn_d), P(z_d), P(y_d), float(f32(theta)), out, None)
    y1, rnorm, zmax = M.post(z1, z, theta)
    assert_bitexact(aos(y_d, shape), y1, "y")
    assert f32(out[0]) == rnorm and f32(out[1]) == zmax, (out[0], rnorm, out[1], zmax)


@pytest.mark.parametrize("dims", [(7, 5, 3), (33, 31, 29)])
def test_stop_test_maxima(lib, dims):
    """where the largest normSquare sits: in the last cell, in the tail behind the last full vector / wave / block, from a negative
    component, tied between two cells, and nowhere (an all-zero grid)"""
    import torch
    sx, sy, sz = dims
    shape, n = (sz, sy, sx), sx * sy * sz
    rng = np.random.RandomState(n + 1)
    base_z, base_z0 = (rng.uniform(-1, 1, (n, 3)).astype(f32) for _ in range(2))

    def run(z, z0):
        y_d, z_d, z0_d = torch.full((3 * n,), float("nan"), device="cuda"), dev(soa(z)), dev(soa(z0))
        out = (ctypes.c_float * 2)()
        lib.call("mf_guiding_post", n, P(z_d), P(z0_d), P(y_d), 0.5, out, None)
        y, rnorm, zmax = M.post(z.reshape(shape + (3,)), z0.reshape(shape + (3,)), 0.5)
        assert_bitexact(aos(y_d, shape), y, "y")
        assert f32(out[0]) == rnorm and f32(out[1]) == zmax, (out[0], rnorm, out[1], zmax)
        return rnorm, zmax

    for cell in (n - 1, n - 2, n - n % 4 if n % 4 else n - 3, (n // 256) * 256, 0):
        z, z0 = base_z.copy(), base_z0.copy()
        z[cell] = (3.5, -4.25, 1.125)
        z0[cell] = (-6.0, 5.0, 0.5)
        rnorm, zmax = run(z, z0)
        assert zmax == M.max_abs(z[cell][None]) and rnorm == M.max_abs((z[cell] - z0[cell])[None])
    z, z0 = base_z.copy(), base_z0.copy()
    z[n // 2] = (0, -9.0, 0)                              # from a negative component alone
    z0[n // 2] = (0, 0, 7.0)
    assert run(z, z0) == (M.max_abs((z[n // 2] - z0[n // 2])[None]), f32(9.0))
    z[3] = (9.0, 0, 0)                                    # tied
    z[n - 1] = (0, 0, -9.0)
    assert run(z, z0)[1] == f32(9.0)
    zero = np.zeros((n, 3), f32)
    assert run(zero, zero) == (f32(0), f32(0))


# ---- the whole plugin ---------------------------------------------------------------------------------------------------------------------
def _solver(m, dims):
    return m.Solver(name="main", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)


def test_all_zero_input_stops_at_iteration_one(lib):
    import manta as m
    s = _solver(m, (12, 10, 9))
    flags, vel, velT, pressure, W = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.MACGrid), s.create(m.RealGrid), s.create(m.RealGrid)
    flags.initDomain(boundaryWidth=1)
    flags.fillGrid()
    W.setConst(1.0)
    m.PD_fluid_guiding(vel=vel, velT=velT, pressure=pressure, flags=flags, weight=W, blurRadius=2)
    st = m.lastGuidingStats()
    assert st["iterations"] == 1 and len(st["cg_iterations"]) == 2 and st["rnorm"] == 0.0
    assert not vel.to_numpy().any()


def _box(m):
    B, I = M.BOX, M.box_inputs()
    s = _solver(m, B["dims"])
    o = dict(flags=s.create(m.FlagGrid), vel=s.create(m.MACGrid), velT=s.create(m.MACGrid), pressure=s.create(m.RealGrid), W=s.create(m.RealGrid))
    o["flags"].from_numpy(I["flags"])
    o["vel"].from_numpy(I["vel"])
    o["velT"].from_numpy(I["velT"])
    o["W"].setConst(1.0)
    m.setGradientYWeight(o["W"], *I["grad"])
    return s, o


@pytest.mark.parametrize("run", list(M.BOX_RUNS))
def test_case_c_obstacle_box(lib, G, run):
    import manta as m
    B, R = M.BOX, M.BOX_RUNS[run]
    s, o = _box(m)
    assert_bitexact(o["W"].to_numpy(), M.box_weight(), "weight")
    m.PD_fluid_guiding(vel=o["vel"], velT=o["velT"], pressure=o["pressure"], flags=o["flags"], weight=o["W"], blurRadius=B["blurRadius"],
                       theta=B["theta"], tau=B["tau"], sigma=B["sigma"], epsRel=B["epsRel"], epsAbs=R["epsAbs"], maxIters=R["maxIters"],
                       preconditioner=B["preconditioner"])
    st = m.lastGuidingStats()
    print(run, st)
    assert st["iterations"] == G[run + "/pd"][0]
    assert st["cg_iterations"] == list(G[run + "/cg"])
    assert_bitexact(o["vel"].to_numpy(), G[run + "/vel"], "vel")
    assert_bitexact(o["pressure"].to_numpy(), G[run + "/pressure"], "pressure")
    assert_bitexact(o["velT"].to_numpy(), M.box_inputs()["velT"], "velT is read only")


def test_single_radius_rule_on_the_device(lib):
    import manta as m
    B = M.BOX
    s, o = _box(m)
    kw = dict(vel=o["vel"], velT=o["velT"], pressure=o["pressure"], flags=o["flags"], weight=o["W"], maxIters=1)
    m.PD_fluid_guiding(blurRadius=2, **kw)
    before = o["vel"].to_numpy().copy()
    with pytest.raises(RuntimeError, match=r"More than a single blur radius not supported at the moment\."):
        m.PD_fluid_guiding(blurRadius=3, **kw)
    assert_bitexact(o["vel"].to_numpy(), before, "a refused call touches nothing")
    m.releaseBlurPrecomp()
    m.PD_fluid_guiding(blurRadius=3, **kw)
    assert m.lastGuidingStats()["iterations"] == 0 and len(m.lastGuidingStats()["cg_iterations"]) == 1


def test_case_a_guiding_2d_loop(lib, G):
    """the main loop of the reference harness's test_1050_guiding2d.py at 40 x 40"""
    import manta as m
    from manta import vec3
    cfg = M.LOOPS["a"]
    res, scale = cfg["dims"][0], cfg["scale"]
    gs = vec3(res, res, 1)
    s = m.Solver(name="main", gridSize=gs, dim=2)
    s.timestep = 2.0 / scale
    flags, vel, velT = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.MACGrid)
    density, pressure, W = s.create(m.RealGrid), s.create(m.RealGrid), s.create(m.RealGrid)
    flags.initDomain(boundaryWidth=1)
    flags.fillGrid()
    source = s.create(m.Cylinder, center=gs * vec3(0.5, 0.3, 0.5), radius=gs.y * 0.14, z=gs * vec3(0, 0.04 * 1.5, 0))
    m.getSpiralVelocity(flags=flags, vel=velT, strength=1.5 * scale)
    m.setGradientYWeight(W=W, minY=0, maxY=res / 2, valAtMin=1, valAtMax=1)
    m.setGradientYWeight(W=W, minY=res / 2, maxY=res, valAtMin=5, valAtMax=5)
    pd, cg = [], []
    for t in range(cfg["steps"]):
        m.resetOutflow(flags=flags, real=density)
        source.applyToGrid(grid=density, value=1)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=density, order=2, clampMode=1)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2, clampMode=1)
        m.setWallBcs(flags=flags, vel=vel)
        m.addBuoyancy(density=density, vel=vel, gravity=vec3(0, 0.25 * scale * -1e-2, 0), flags=flags)
        m.PD_fluid_guiding(vel=vel, velT=velT, flags=flags, weight=W, blurRadius=cfg["blurRadius"], pressure=pressure, tau=cfg["tau"],
                           sigma=cfg["sigma"], theta=cfg["theta"], epsRel=cfg["epsRel"], epsAbs=cfg["epsAbs"], preconditioner=cfg["preconditioner"])
        st = m.lastGuidingStats()
        pd.append(st["iterations"])
        cg += st["cg_iterations"]
        m.setWallBcs(flags=flags, vel=vel)
        s.step()
    print("a: pd", pd, "reference", list(G["a/pd"]))
    assert pd == list(G["a/pd"])
    assert cg == list(G["a/cg"])
    assert_bitexact(vel.to_numpy(), G["a/vel"], "vel")
    assert_bitexact(density.to_numpy(), G["a/density"], "density")
    assert_bitexact(pressure.to_numpy(), G["a/pressure"], "pressure")


def _loop_b(m, cfg, steps):
    from manta import vec3
    res2, factor = cfg["dims"][0], cfg["factor"]
    gs2 = vec3(res2, int(2.0 * res2), res2)
    s2 = m.Solver(name="main", gridSize=gs2, dim=3)
    s2.timestep = cfg["timestep"]
    flags, vel, velT = s2.create(m.FlagGrid), s2.create(m.MACGrid), s2.create(m.MACGrid)
    density, pressure, W = s2.create(m.RealGrid), s2.create(m.RealGrid), s2.create(m.RealGrid)
    noise = s2.create(m.NoiseField, loadFromFile=True)
    noise.posScale = vec3(0)
    noise.clamp = True
    noise.clampNeg = 0
    noise.clampPos = 1
    noise.valScale = 1
    noise.valOffset = 0.75
    noise.timeAnim = 0.2
    flags.initDomain(boundaryWidth=0)
    flags.fillGrid()
    m.setOpenBound(flags, 0, "yY", m.FlagOutflow | m.FlagEmpty)
    source = s2.create(m.Cylinder, center=gs2 * vec3(0.5, 0.05, 0.5), radius=res2 * 0.1, z=gs2 * vec3(0, 0.02, 0))
    W.multConst(0)
    W.addConst(cfg["wScalar"])
    pd, cg, mgs = [], [], []
    for t in range(steps):
        m.densityInflow(flags=flags, density=density, noise=noise, shape=source, scale=1, sigma=0.5)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=density, order=2)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2)
        m.resetOutflow(flags=flags, real=density)
        m.setWallBcs(flags=flags, vel=vel)
        m.addBuoyancy(density=density, vel=vel, gravity=vec3(0, -1e-3 * factor, 0), flags=flags)
        m.getSpiralVelocity(flags=flags, vel=velT, strength=1.0, with3D=True)
        velT.multConst(vec3(factor))
        m.PD_fluid_guiding(vel=vel, velT=velT, flags=flags, weight=W, blurRadius=cfg["blurRadius"], pressure=pressure, tau=cfg["tau"],
                           sigma=cfg["sigma"], theta=cfg["theta"], epsRel=cfg["epsRel"], epsAbs=cfg["epsAbs"], preconditioner=m.PcMGStatic,
                           zeroPressureFixing=True)
        st = m.lastGuidingStats()
        pd.append(st["iterations"])
        cg += st["cg_iterations"]
        mgs.append(s2._mg)
        m.setWallBcs(flags=flags, vel=vel)
        s2.step()
    return s2, pd, cg, mgs, vel, density, pressure


def test_case_b_guiding_3d_loop_and_release_mg(lib, G):
    """the main loop of scenes/guiding_3d02_high.py at 16 x 32 x 16 with a spiral target; the calls of both steps share the solver's
    one multigrid hierarchy (PcMGStatic), and releaseMG(solver) afterwards lets go of it"""
    import manta as m
    cfg = M.LOOPS["b"]
    s2, pd, cg, mgs, vel, density, pressure = _loop_b(m, cfg, cfg["steps"])
    print("b: pd", pd, "reference", list(G["b/pd"]))
    assert pd == list(G["b/pd"])
    assert cg == list(G["b/cg"])
    assert_bitexact(vel.to_numpy(), G["b/vel"], "vel")
    assert_bitexact(density.to_numpy(), G["b/density"], "density")
    assert_bitexact(pressure.to_numpy(), G["b/pressure"], "pressure")
    assert mgs[0] is not None and all(h is mgs[0] for h in mgs)
    assert mgs[0].info()["setups"] == 1, mgs[0].info()          # many inner solves, one set-up
    m.releaseMG(s2)
    assert s2._mg is None and mgs[0].handle is None
    m.releaseMG(s2)                                             # and again: nothing left to release
