"""Fill-fraction obstacle boundaries, CPU side: the numpy model (tests/obstacle_model.py) against the recorded reference outputs
in tests/golden/obstacles.npz, the public names, and the clear refusal of a backend without the extension.

tests/golden/obstacles.npz holds reference outputs only; the inputs are regenerated from obstacle_model.case_inputs(name) /
obstacle_model.loop_inputs(dims).  They were recorded from the reference (zoharl3/mantaflow, float Real, compiled as oracle/ref.mk
compiles it) run with OMP_NUM_THREADS=1, one call per array:

  uf_*                  updateFractions(flags, phiObs, fractions, boundaryWidth=bw, fracThreshold=0.01)            -> fractions
  sof_*                 setObstacleFlags(flags, phiObs, fractions?, phiOut?, phiIn?, boundaryWidth=bw)             -> flags
  wbf_*                 setWallBcs(flags, vel, fractions=<any grid>, phiObs=phiObs)                                -> vel
  infl_*                setInflowBcs(vel, dir, value)                                                              -> vel
  noise_*               addNoise(flags, density, noise, sdf?, scale) with NoiseField(fixedSeed=-1), posScale 75, clamp to
                        [-1, 1] (obstacle_model.NOISE)                                                             -> density
  loop2d__*, loop3d__*  updateFractions(boundaryWidth=0), setObstacleFlags(fractions), flags.fillGrid(), then per step
                        advectSemiLagrange(vel, vel, order=2), extrapolateMACSimple(distance=2, intoObs=True),
                        setWallBcs(fractions, phiObs), setInflowBcs("xX", (0.9, 0, 0)),
                        solvePressure(fractions, cgAccuracy=1e-4, cgMaxIterFac=5)  (obstacle_model.LOOPS: 128x64 2-D,
                        10 steps; 48x32x32, 5 steps) -> flags, fractions, vel, pressure, and the CG iterations of each step
"""
import os

import numpy as np
import pytest

import obstacle_model as M
import util

GOLDEN = np.load(os.path.join(util.GOLDEN, "obstacles.npz"))
NAMES = ("updateFractions", "setObstacleFlags", "setInflowBcs", "addNoise", "setWallBcs")


def noise_tile_and_params(dims):
    """the wavelet noise tile and the 20-float parameter block of the addNoise cases, from the package on the current backend"""
    import manta as m
    s = m.Solver(name="n", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)
    noise = s.create(m.NoiseField, loadFromFile=True)
    noise.posScale = m.vec3(M.NOISE["posScale"])
    noise.clamp, noise.clampNeg, noise.clampPos = M.NOISE["clamp"], M.NOISE["clampNeg"], M.NOISE["clampPos"]
    return noise._tile.detach().cpu().numpy(), np.array(list(noise._params()), np.float32), (s, noise)


@pytest.mark.parametrize("name", [n for n, c in M.CASES.items() if c[0] != "addNoise"])
def test_model_equals_reference_fixture(name):
    util.assert_bitexact(M.model_case(name), GOLDEN[name], name)


@pytest.mark.parametrize("name", [n for n, c in M.CASES.items() if c[0] == "addNoise"])
def test_model_add_noise_equals_reference_fixture(oracle_backend, name):
    tile, params, _ = noise_tile_and_params(M.CASES[name][1])
    util.assert_bitexact(M.model_case(name, tile, params), GOLDEN[name], name)


def test_update_fractions_fixture_exercises_the_serial_order_and_the_z_quirk():
    """the "max z" rule's 1s survive on the last plane (outside the bnd=1 range), and only in rows j >= sz - w - 2"""
    name = "uf_20x13x11_w0"
    x = M.case_inputs(name)
    fr = GOLDEN[name]
    sz, sy, sx = x["flags"].shape
    top = fr[:, sz - 1]
    assert top.any()
    jj = np.nonzero(top[0])[0]
    assert jj.min() >= sz - 2   # boundaryWidth 0


def test_loop_fixtures_are_consistent():
    for name, cfg in M.LOOPS.items():
        it = GOLDEN[name + "__iterations"]
        assert it.shape == (cfg["steps"],) and (it > 0).all()
        f, phi, _ = M.loop_inputs(cfg["dims"])
        fr = M.update_fractions(f, phi, 0)
        util.assert_bitexact(fr, GOLDEN[name + "__fractions"], name + " fractions")
        fl = M.set_obstacle_flags(f, phi, fr, boundaryWidth=1)
        keep = (fl & (M.OBSTACLE | M.INFLOW | M.OUTFLOW | M.OPEN)) != 0
        fl = np.where(keep, fl, (fl & ~(M.EMPTY | M.FLUID)) | M.FLUID)
        util.assert_bitexact(fl, GOLDEN[name + "__flags"], name + " flags")


def test_fixture_file_is_small():
    assert os.path.getsize(os.path.join(util.GOLDEN, "obstacles.npz")) < 1 << 20


def test_manta_exports_the_obstacle_plugins():
    import manta
    ns = {}
    exec("from manta import *", ns)
    for n in NAMES:
        assert callable(ns[n]), n
        assert getattr(manta, n) is ns[n]


def test_backend_without_extension_refuses_clearly(oracle_backend):
    import manta as m
    from mantaflow_amd import _lib
    assert _lib.get().obstacles is False
    s = m.Solver(name="o", gridSize=m.vec3(12, 10, 8), dim=3)
    flags, vel, fr = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.MACGrid)
    phi, dens = s.create(m.LevelsetGrid), s.create(m.RealGrid)
    flags.initDomain()
    noise = s.create(m.NoiseField, loadFromFile=True)
    calls = {
        "updateFractions": lambda: m.updateFractions(flags=flags, phiObs=phi, fractions=fr),
        "setObstacleFlags": lambda: m.setObstacleFlags(flags=flags, phiObs=phi, fractions=fr),
        "setWallBcs": lambda: m.setWallBcs(flags=flags, vel=vel, fractions=fr, phiObs=phi),
        "setInflowBcs": lambda: m.setInflowBcs(vel=vel, dir="xX", value=m.vec3(1, 0, 0)),
        "addNoise": lambda: m.addNoise(flags=flags, density=dens, noise=noise),
    }
    for name, fn in calls.items():
        with pytest.raises(RuntimeError, match=r"%s: the 'oracle' backend does not implement" % name):
            fn()
    m.setWallBcs(flags=flags, vel=vel)                 # the plain mode is untouched
    m.setWallBcs(flags=flags, vel=vel, phiObs=phi)     # phiObs alone (movingObstacle.py) is the plain mode too


def test_header_declares_the_extension():
    from mantaflow_amd import _lib
    protos = _lib.parse_header(_lib.OBSTACLES_HEADER)
    for n in ("mf_obstacles_abi_version", "mf_update_fractions", "mf_set_obstacle_flags", "mf_set_wall_bcs_frac",
              "mf_set_wall_bcs_frac_scratch_words", "mf_set_inflow_bcs", "mf_add_noise"):
        assert n in protos, n
    assert not set(protos) & set(_lib.parse_header())


def test_inflow_bad_character_message():
    v = M.rand_mac((6, 5, 4), 0)
    with pytest.raises(RuntimeError, match=r"invalid character in direction string\. Only \[xyzXYZ\] allowed\."):
        M.set_inflow_bcs(v, "xQ", (1, 0, 0))
