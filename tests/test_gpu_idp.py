"""GPU: implicit density projection through the package on the HIP backend, against the reference fixture tests/golden/idp.npz (how
each array was produced: tests/test_idp_model.py), against the numpy model on seeded random inputs, and the scenes' loop against
recorded reference runs.  Everything is compared bit for bit."""
import os

import numpy as np
import pytest

import idp_model as M
import util

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idp.npz"))


def _solver(m, dims):
    return m.Solver(name="t", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)


def _parts(m, s, pos, pflag, ptype=None):
    pp = s.create(m.BasicParticleSystem)
    pp.set_positions(pos, pflag)
    pt = None
    if ptype is not None:
        pt = pp.create(m.PdataInt)
        pt.from_numpy(ptype)
    return pp, pt


def _grid(s, cls, arr):
    g = s.create(cls)
    g.from_numpy(arr)
    return g


def run_case(m, kind, dims, I, opt):
    """one plugin call through the package; returns the outputs under the fixture's array names (and the stats)"""
    from mantaflow_amd import plugins
    s = _solver(m, dims)
    if kind == "mark":
        pp, pt = _parts(m, s, I["pos"], I["pflag"], I["ptype"] if opt["ptype"] else None)
        flags, phi, dX = _grid(s, m.FlagGrid, I["flags"]), _grid(s, m.LevelsetGrid, I["phiObs"]), s.create(m.MACGrid)
        dX.setConst(m.vec3(9, 9, 9))       # cleared by the plugin
        m.markFluidAndBoundaryCells(particles=pp, flags=flags, deltaX=dX, phiObs=phi, ptype=pt, exclude=I["exclude"] if opt["ptype"] else 0)
        return dict(flags=flags.to_numpy(), deltaX=dX.to_numpy()), dict(plugins.markFluidAndBoundaryCellsStats)
    if kind == "mass":
        pp, _ = _parts(m, s, I["pos"], I["pflag"])
        src = pp.create(m.PdataReal)
        flags, phi, dX, dens = _grid(s, m.FlagGrid, I["flags"]), _grid(s, m.LevelsetGrid, I["phiObs"]), s.create(m.MACGrid), s.create(m.RealGrid)
        dens.setConst(7.0)
        m.mapMassToGrid(flags=flags, density=dens, parts=pp, source=src, deltaX=dX, phiObs=phi, dt=I["dt"], particleMass=I["mass"],
                        noDensityClamping=opt["noClamp"])
        return dict(flags=flags.to_numpy(), density=dens.to_numpy(), deltaX=dX.to_numpy()), dict(plugins.mapMassToGridStats)
    if kind == "delta":
        flags, dX, L = _grid(s, m.FlagGrid, I["flags"]), _grid(s, m.MACGrid, I["deltaX"]), _grid(s, m.RealGrid, I["Lambda"])
        m.computeDeltaX(deltaX=dX, Lambda=L, flags=flags)
        assert np.array_equal(flags.to_numpy(), I["flags"])
        return dict(deltaX=dX.to_numpy(), Lambda=L.to_numpy()), {}
    pp, pt = _parts(m, s, I["pos"], I["pflag"], I["ptype"] if opt["ptype"] else None)
    flags, dX = s.create(m.FlagGrid), _grid(s, m.MACGrid, I["deltaX"])
    m.mapMACToPartPositions(flags=flags, deltaX=dX, parts=pp, dt=I["dt"], ptype=pt, exclude=I["exclude"] if opt["ptype"] else 0, mapQuadratic=True)
    return dict(pos=pp.get_positions()), {}


@pytest.mark.parametrize("name", list(M.CASES))
def test_hip_equals_the_reference_fixture(hip_backend, name):
    import manta as m
    kind, dims, seed, opt = M.CASES[name]
    out, stats = run_case(m, kind, dims, M.case_inputs(name), opt)
    for k, v in out.items():
        util.assert_bitexact(v, GOLDEN[name + "/" + k], name + "/" + k)
    if kind in ("mark", "mass"):
        _, info = M.model_case(name)
        assert stats["boundary_particles"] == info["boundary"] and stats["pushing"] == info["pushing"]
    if kind == "mass":
        assert stats["flipped"] == info["flipped"] and stats["candidates"] == info["candidates"]
        assert stats["readbacks"] <= 3


def test_copy_flags_to_flags(hip_backend):
    import manta as m
    s = _solver(m, (13, 11, 9))
    src = np.random.RandomState(3).randint(0, 128, (9, 11, 13)).astype(np.int32)
    a, b = _grid(s, m.FlagGrid, src), s.create(m.FlagGrid)
    m.copyFlagsToFlags(a, b)
    assert np.array_equal(b.to_numpy(), src)


# sizes whose rows are not a multiple of 8 cells among them; the largest holds a few hundred thousand particles
RANDOM = [("mass", (37, 29, 23), 101, dict(noClamp=False)), ("mass", (64, 48, 40), 102, dict(noClamp=True)),
          ("mass", (61, 50, 1), 103, dict(noClamp=False)), ("mass", (130, 67, 1), 104, dict(noClamp=True)),
          ("mark", (37, 29, 23), 105, dict(ptype=True)), ("mark", (45, 31, 1), 106, dict(ptype=True)),
          ("delta", (37, 29, 23), 107, {}), ("delta", (61, 50, 1), 108, {}),
          ("pos", (37, 29, 23), 109, dict(ptype=True)), ("pos", (61, 50, 1), 110, dict(ptype=True))]


@pytest.mark.parametrize("kind,dims,seed,opt", RANDOM, ids=["%s-%dx%dx%d" % (r[0], *r[1]) for r in RANDOM])
def test_hip_equals_the_model_on_random_inputs(hip_backend, kind, dims, seed, opt):
    import manta as m
    if kind == "mark":
        I = M.mark_inputs(dims, seed, n=60000)
    elif kind == "pos":
        I = M.position_inputs(dims, seed, n=200000)
    else:
        I = M.INPUTS[kind](dims, seed)
    out, stats = run_case(m, kind, dims, I, opt)
    if kind == "mark":
        fl, dX, info = M.mark_fluid_and_boundary(I["pos"], I["pflag"], I["flags"], I["phiObs"], I["ptype"], I["exclude"])
        want = dict(flags=fl, deltaX=dX)
        assert stats["boundary_particles"] == info["boundary"] > 1000 and stats["pushing"] == info["pushing"]
    elif kind == "mass":
        fl, d, dX, st = M.map_mass_to_grid(I["flags"], I["pos"], I["pflag"], I["phiObs"], I["dt"], I["mass"], opt["noClamp"])
        want = dict(flags=fl, density=d, deltaX=dX)
        print("particles %d, stats %s" % (len(I["pflag"]), stats))
        assert stats["flipped"] == st["flipped"] > 0 and stats["boundary_particles"] == st["boundary"] > 0
        assert stats["candidates"] == st["candidates"] and stats["rounds"] == st["rounds"]
    elif kind == "delta":
        dX, L = M.compute_delta_x(I["deltaX"], I["Lambda"], I["flags"])
        want = dict(deltaX=dX, Lambda=L)
    else:
        want = dict(pos=M.map_mac_to_part_positions(dims, I["deltaX"], I["pos"], I["pflag"], I["dt"], I["ptype"], I["exclude"]))
    for k, v in want.items():
        util.assert_bitexact(out[k], v, "%s %s" % (kind, k))


@pytest.mark.parametrize("name", list(M.LOOPS))
def test_scene_loop_equals_the_recorded_reference_run(hip_backend, name):
    """the main loop of scenes/idp_apic01_simple.py / idp_apic02_3d.py (idp_model.idp_loop: same calls and arguments) on a small dam
    break with adaptive time stepping: per step dt and the CG iterations of both solves, at the end every field and every n-th
    particle.  The model, fed with each step's inputs, vouches that the run exercises the push-out and the flips."""
    import manta as m
    cfg = M.LOOPS[name]
    seen = dict(boundary=0, pushing=0, flipped=0, steps_with_boundary=0, steps_with_flips=0)

    def before_mass(t, flagsPos, pp, phiObs, dt, mass):
        _, _, _, st = M.map_mass_to_grid(flagsPos.to_numpy(), pp.get_positions(), pp.get_flags(), phiObs.to_numpy(), dt, mass)
        seen["boundary"] += st["boundary"]
        seen["pushing"] += st["pushing"]
        seen["flipped"] += st["flipped"]
        seen["steps_with_boundary"] += st["boundary"] > 0
        seen["steps_with_flips"] += st["flipped"] > 0

    out = M.idp_loop(m, cfg["res"], cfg["dim"], cfg["steps"], cfl=cfg["cfl"], before_mass=before_mass)
    print(name, seen, "dt", out["dt"], "it_pos", out["it_pos"], "it_vel", out["it_vel"])
    assert seen["steps_with_flips"] >= 1, seen
    if cfg["dim"] == 3:
        # the 2-D dam break never puts a particle into a wall (the reference run: none in 150 steps at three resolutions); the 3-D one does
        assert seen["steps_with_boundary"] >= 1 and seen["pushing"] >= 1, seen
    assert sum(s["boundary_particles"] for s in out["stats"]) == seen["boundary"] and sum(s["flipped"] for s in out["stats"]) == seen["flipped"]
    assert len(np.unique(GOLDEN[name + "/dt"])) > 3, "the recorded dt never varied"
    util.assert_bitexact(out["dt"], GOLDEN[name + "/dt"], "dt per step")
    assert np.array_equal(out["it_pos"], GOLDEN[name + "/it_pos"]), (out["it_pos"], GOLDEN[name + "/it_pos"])
    assert np.array_equal(out["it_vel"], GOLDEN[name + "/it_vel"]), (out["it_vel"], GOLDEN[name + "/it_vel"])
    assert out["np"][0] == GOLDEN[name + "/np"][0]
    for k in ("density", "Lambda", "deltaX", "flags", "flagsPos", "vel", "pos"):
        util.assert_bitexact(out[k], GOLDEN[name + "/" + k], name + "/" + k)
