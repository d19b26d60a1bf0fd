"""Fill-fraction obstacle boundaries on the MI355X: every HIP entry of include/manta_hip_obstacles.h against the recorded reference
outputs (tests/golden/obstacles.npz, see tests/test_obstacles_model.py for how each array was produced) and against the numpy
model (tests/obstacle_model.py) on seeded inputs; the two obstacle loops against the reference; a moving-obstacle loop."""
import ctypes
import os

import numpy as np
import pytest
import torch

import obstacle_model as M
import util

GOLDEN = np.load(os.path.join(util.GOLDEN, "obstacles.npz"))

pytestmark = pytest.mark.gpu


def _solver(m, dims):
    return m.Solver(name="obs", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)


def _grid(s, cls, arr):
    g = s.create(cls)
    g.from_numpy(arr if arr.ndim == 3 else np.moveaxis(arr, 0, -1))
    return g


def _np(g):
    a = g.to_numpy()
    return np.ascontiguousarray(np.moveaxis(a, -1, 0)) if a.ndim == 4 else a


def run_pkg(plugin, dims, x, a):
    """one plugin call through the package on the active backend; returns its output as numpy"""
    import manta as m
    s = _solver(m, dims)
    if plugin == "updateFractions":
        flags, phi, fr = _grid(s, m.FlagGrid, x["flags"]), _grid(s, m.RealGrid, x["phi"]), s.create(m.MACGrid)
        fr.setConst(m.vec3(7.0))   # every face is written
        m.updateFractions(flags=flags, phiObs=phi, fractions=fr, boundaryWidth=a["bw"])
        return _np(fr)
    if plugin == "setObstacleFlags":
        flags, phi = _grid(s, m.FlagGrid, x["flags"]), _grid(s, m.RealGrid, x["phi"])
        kw = {k: _grid(s, m.MACGrid if k == "fractions" else m.RealGrid, x[k]) for k in ("fractions", "phiOut", "phiIn") if k in x}
        m.setObstacleFlags(flags=flags, phiObs=phi, boundaryWidth=a["bw"], **kw)
        return _np(flags)
    if plugin == "setWallBcs":
        flags, phi, vel = _grid(s, m.FlagGrid, x["flags"]), _grid(s, m.RealGrid, x["phi"]), _grid(s, m.MACGrid, x["vel"])
        fr = s.create(m.MACGrid)
        m.setWallBcs(flags=flags, vel=vel, fractions=fr, phiObs=phi)
        return _np(vel)
    if plugin == "setInflowBcs":
        vel = _grid(s, m.MACGrid, x["vel"])
        m.setInflowBcs(vel=vel, dir=a["dir"], value=m.vec3(*a["value"]))
        return _np(vel)
    if plugin == "addNoise":
        flags, dens = _grid(s, m.FlagGrid, x["flags"]), _grid(s, m.RealGrid, x["density"])
        noise = s.create(m.NoiseField, loadFromFile=True)
        noise.posScale = m.vec3(M.NOISE["posScale"])
        noise.clamp, noise.clampNeg, noise.clampPos = M.NOISE["clamp"], M.NOISE["clampNeg"], M.NOISE["clampPos"]
        sdf = _grid(s, m.RealGrid, x["sdf"]) if "sdf" in x else None
        m.addNoise(flags=flags, density=dens, noise=noise, sdf=sdf, scale=a["scale"])
        return _np(dens), noise._tile.detach().cpu().numpy(), np.array(list(noise._params()), np.float32)
    raise KeyError(plugin)


@pytest.mark.parametrize("name", list(M.CASES))
def test_hip_equals_reference_fixture(hip_backend, name):
    plugin, dims, _, a = M.CASES[name]
    got = run_pkg(plugin, dims, M.case_inputs(name), a)
    util.assert_bitexact(got[0] if plugin == "addNoise" else got, GOLDEN[name], name)


SIZES = [(16, 16, 16), (20, 13, 11), (37, 29, 1), (64, 48, 40), (21, 19, 13), (45, 23, 1)]


@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("seed", [31, 32])
def test_hip_equals_model_random(hip_backend, dims, seed):
    is3d = dims[2] > 1
    sides = ("iopwpp", "pwioop")[seed % 2] if is3d else ("iopw", "opip")[seed % 2]
    for bw in (0, 1):
        f, phi = M.scene_inputs(dims, seed + 10 * bw, sides, bw)
        x = dict(flags=f, phi=phi)
        util.assert_bitexact(run_pkg("updateFractions", dims, x, dict(bw=bw)), M.update_fractions(f, phi, bw), "updateFractions bw=%d" % bw)
    fr = M.update_fractions(f, phi, 1)
    rng = np.random.RandomState(seed)
    po, pi = rng.uniform(-1, 1, f.shape).astype(np.float32), rng.uniform(-1, 1, f.shape).astype(np.float32)
    for kw in (dict(fractions=fr), dict(), dict(fractions=fr, phiOut=po, phiIn=pi)):
        for bw in ((1, 2) if "fractions" in kw else (0, 1)):
            want = M.set_obstacle_flags(f, phi, kw.get("fractions"), kw.get("phiOut"), kw.get("phiIn"), bw)
            util.assert_bitexact(run_pkg("setObstacleFlags", dims, dict(flags=f, phi=phi, **kw), dict(bw=bw)), want, "setObstacleFlags")
    fw, phiw = M.scene_inputs(dims, seed + 5, "wwwwww", 0, fluid_frac=0.7)
    vel = M.rand_mac(dims, seed)
    util.assert_bitexact(run_pkg("setWallBcs", dims, dict(flags=fw, phi=phiw, vel=vel), {}), M.set_wall_bcs_frac(fw, vel, phiw),
                         "setWallBcs frac")
    for d in ("xX", "yZ", "zYx"):
        a = dict(dir=d, value=(0.5, -1.25, 3.0))
        util.assert_bitexact(run_pkg("setInflowBcs", dims, dict(vel=vel), a), M.set_inflow_bcs(vel, d, a["value"]), "setInflowBcs " + d)
    dens = rng.uniform(0, 1, f.shape).astype(np.float32)
    got, tile, params = run_pkg("addNoise", dims, dict(flags=f, density=dens, sdf=phi), dict(scale=0.3))
    util.assert_bitexact(got, M.add_noise(f, dens, tile, params, phi, 0.3), "addNoise")


def test_hip_wall_bcs_frac_256_sphere(hip_backend):
    """the per-step hot path at 256^3 around a sphere of radius 0.2 * res (plus the domain walls)"""
    res = 256
    dims = (res, res, res)
    shape = (res, res, res)
    k, j, i = np.meshgrid(*(np.arange(res, dtype=np.float32),) * 3, indexing="ij")
    phi = (np.sqrt((i + 0.5 - 0.5 * res) ** 2 + (j + 0.5 - 0.5 * res) ** 2 + (k + 0.5 - 0.5 * res) ** 2) - 0.2 * res).astype(np.float32)
    del i, j, k
    f = np.where(phi < 0, M.OBSTACLE, M.FLUID).astype(np.int32)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = (M.OBSTACLE,) * 6
    vel = M.rand_mac(dims, 3)
    got = run_pkg("setWallBcs", dims, dict(flags=f, phi=phi, vel=vel), {})
    want = M.set_wall_bcs_frac(f, vel, phi)
    assert not np.array_equal(want, vel)
    util.assert_bitexact(got, want, "setWallBcs frac 256^3")
    assert shape == f.shape


def _loop_pkg(dims, steps):
    import manta as m
    from mantaflow_amd import plugins
    f, phi, vel0 = M.loop_inputs(dims)
    s = _solver(m, dims)
    flags, phiObs, vel = _grid(s, m.FlagGrid, f), _grid(s, m.LevelsetGrid, phi), _grid(s, m.MACGrid, vel0)
    fractions, pressure = s.create(m.MACGrid), s.create(m.RealGrid)
    m.updateFractions(flags=flags, phiObs=phiObs, fractions=fractions)
    m.setObstacleFlags(flags=flags, phiObs=phiObs, fractions=fractions)
    flags.fillGrid()
    inflow = m.vec3(*M.LOOP_INFLOW)
    iters = []
    for _ in range(steps):
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2)
        m.extrapolateMACSimple(flags=flags, vel=vel, distance=2, intoObs=True)
        m.setWallBcs(flags=flags, vel=vel, fractions=fractions, phiObs=phiObs)
        m.setInflowBcs(vel=vel, dir="xX", value=inflow)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure, fractions=fractions, **M.LOOP_CG)
        iters.append(plugins.lastCgStats()["iterations"])
    return dict(flags=_np(flags), fractions=_np(fractions), vel=_np(vel), pressure=_np(pressure), iterations=np.array(iters, np.int32))


@pytest.mark.parametrize("name", list(M.LOOPS))
def test_hip_obstacle_loop_equals_reference(hip_backend, name):
    """flags and fractions bit-exact, identical CG iteration counts at every step, vel / pressure within 1e-5 relative"""
    cfg = M.LOOPS[name]
    got = _loop_pkg(cfg["dims"], cfg["steps"])
    util.assert_bitexact(got["flags"], GOLDEN[name + "__flags"], name + " flags")
    util.assert_bitexact(got["fractions"], GOLDEN[name + "__fractions"], name + " fractions")
    assert got["iterations"].tolist() == GOLDEN[name + "__iterations"].tolist()
    errs = {k: util.rel_err(got[k], GOLDEN[name + "__" + k]) for k in ("vel", "pressure")}
    exact = {k: np.array_equal(got[k].view(np.int32), GOLDEN[name + "__" + k].view(np.int32)) for k in ("vel", "pressure")}
    print("%s: rel err %s, bit-exact %s" % (name, errs, exact))
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)


def test_hip_moving_obstacle_loop(hip_backend):
    """movingObstacle.py-style: the flags are rebuilt from a moving sphere with setObstacleFlags every step (and the fractions with
    updateFractions), followed by the fraction-mode wall BCs; every step equals the model chain"""
    import manta as m
    dims = (40, 32, 24)
    sx, sy, sz = dims
    s = _solver(m, dims)
    flags, phiObs, fr = s.create(m.FlagGrid), s.create(m.LevelsetGrid), s.create(m.MACGrid)
    vel = _grid(s, m.MACGrid, M.rand_mac(dims, 9, 0.5))
    want_v = M.rand_mac(dims, 9, 0.5)
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    f0 = np.full((sz, sy, sx), M.EMPTY, np.int32)
    f0[:, :, 0] = f0[:, :, -1] = f0[:, 0] = f0[:, -1] = f0[0] = f0[-1] = M.OBSTACLE
    flags.from_numpy(f0)
    want_f = f0
    for t in range(6):
        c = (0.3 * sx + 2.5 * t, 0.5 * sy, 0.5 * sz)
        phi = (np.sqrt((i + 0.5 - c[0]) ** 2 + (j + 0.5 - c[1]) ** 2 + (k + 0.5 - c[2]) ** 2) - 0.2 * sy).astype(np.float32)
        phiObs.from_numpy(phi)
        m.setObstacleFlags(flags=flags, phiObs=phiObs)
        flags.fillGrid()
        m.updateFractions(flags=flags, phiObs=phiObs, fractions=fr, boundaryWidth=0)
        m.setWallBcs(flags=flags, vel=vel, fractions=fr, phiObs=phiObs)
        want_f = M.set_obstacle_flags(want_f, phi, boundaryWidth=1)
        keep = (want_f & (M.OBSTACLE | M.INFLOW | M.OUTFLOW | M.OPEN)) != 0
        want_f = np.where(keep, want_f, (want_f & ~(M.EMPTY | M.FLUID)) | M.FLUID).astype(np.int32)
        want_fr = M.update_fractions(want_f, phi, 0)
        want_v = M.set_wall_bcs_frac(want_f, want_v, phi)
        util.assert_bitexact(_np(flags), want_f, "flags step %d" % t)
        util.assert_bitexact(_np(fr), want_fr, "fractions step %d" % t)
        util.assert_bitexact(_np(vel), want_v, "vel step %d" % t)


def test_hip_library_exports_every_obstacle_symbol():
    from mantaflow_amd import _lib
    L = ctypes.CDLL(util.HIP_LIB)
    for name in _lib.parse_header(_lib.OBSTACLES_HEADER):
        assert hasattr(L, name), name
    assert L.mf_obstacles_abi_version() == 1


def test_hip_inflow_bad_character_applies_the_prefix_then_raises(hip_backend):
    import manta as m
    dims = (12, 10, 8)
    s = _solver(m, dims)
    v0 = M.rand_mac(dims, 4)
    vel = _grid(s, m.MACGrid, v0)
    with pytest.raises(RuntimeError, match=r"invalid character in direction string\. Only \[xyzXYZ\] allowed\."):
        m.setInflowBcs(vel=vel, dir="xQ", value=m.vec3(1, 2, 3))
    util.assert_bitexact(_np(vel), M.set_inflow_bcs(v0, "x", (1, 2, 3)), "prefix applied")
