"""Public surface of implicit density projection, on the CPU checker backend: names and signatures of the reference, the refusals
(before anything is touched), copyFlagsToFlags, and -- where the reference's scenes are at hand -- that every call of the two IDP
scenes binds against the package's signatures."""
import ast
import inspect
import os

import numpy as np
import pytest

import idp_model as M

SCENES = "/root/reference/scenes"


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def test_public_names_and_signatures():
    import manta as m
    E = inspect.Parameter.empty
    assert _params(m.copyFlagsToFlags) == [("source", E), ("target", E)]
    assert _params(m.markFluidAndBoundaryCells) == [("particles", E), ("flags", E), ("deltaX", E), ("phiObs", E), ("ptype", None), ("exclude", 0)]
    assert _params(m.mapMassToGrid) == [("flags", E), ("density", E), ("parts", E), ("source", E), ("deltaX", E), ("phiObs", E), ("dt", E),
                                        ("particleMass", E), ("noDensityClamping", False)]
    assert _params(m.computeDeltaX) == [("deltaX", E), ("Lambda", E), ("flags", E)]
    assert _params(m.mapMACToPartPositions) == [("flags", E), ("deltaX", E), ("parts", E), ("dt", E), ("ptype", None), ("exclude", 0),
                                                ("mapQuadratic", False)]
    ns = {}
    exec("from manta import *", ns)
    for n in ("copyFlagsToFlags", "markFluidAndBoundaryCells", "mapMassToGrid", "computeDeltaX", "mapMACToPartPositions"):
        assert n in ns


def test_header_declares_the_extension():
    from mantaflow_amd import _lib
    protos = _lib.parse_header(_lib.IDP_HEADER)
    for n in ("mf_idp_abi_version", "mf_idp_mark", "mf_idp_map_weights", "mf_idp_compute_density", "mf_idp_compute_delta_x",
              "mf_idp_map_mac_to_positions"):
        assert n in protos, n
    for other in [_lib.HEADER] + [e.header for e in _lib.EXTENSIONS if e.name != "idp"]:
        assert not set(protos) & set(_lib.parse_header(other))


def _objects(m, s):
    pp = s.create(m.BasicParticleSystem)
    pp.set_positions(np.random.RandomState(0).uniform(1, 7, (50, 3)))
    o = dict(pp=pp, pMass=pp.create(m.PdataReal), flags=s.create(m.FlagGrid), deltaX=s.create(m.MACGrid), phiObs=s.create(m.LevelsetGrid),
             density=s.create(m.RealGrid), Lambda=s.create(m.RealGrid))
    o["flags"].initDomain(boundaryWidth=1)
    o["flags"].fillGrid()
    o["deltaX"].setConst(m.vec3(1, 2, 3))
    o["density"].setConst(4.0)
    o["Lambda"].setConst(5.0)
    return o


def _refused(m, o, pattern):
    before = {k: (v.get_positions().copy() if k == "pp" else v.to_numpy().copy()) for k, v in o.items()}
    with pytest.raises(RuntimeError, match=r"markFluidAndBoundaryCells: " + pattern):
        m.markFluidAndBoundaryCells(particles=o["pp"], flags=o["flags"], deltaX=o["deltaX"], phiObs=o["phiObs"])
    with pytest.raises(RuntimeError, match=r"mapMassToGrid: " + pattern):
        m.mapMassToGrid(flags=o["flags"], density=o["density"], parts=o["pp"], source=o["pMass"], deltaX=o["deltaX"], phiObs=o["phiObs"], dt=0.5,
                        particleMass=0.125)
    with pytest.raises(RuntimeError, match=r"computeDeltaX: " + pattern):
        m.computeDeltaX(deltaX=o["deltaX"], Lambda=o["Lambda"], flags=o["flags"])
    with pytest.raises(RuntimeError, match=r"mapMACToPartPositions: " + pattern):
        m.mapMACToPartPositions(flags=o["flags"], deltaX=o["deltaX"], parts=o["pp"], dt=0.5)
    for k, v in o.items():      # nothing was touched
        assert np.array_equal(v.get_positions() if k == "pp" else v.to_numpy(), before[k]), k


def test_cpu_backend_refuses_the_plugins(oracle_backend):
    import manta as m
    from mantaflow_amd import _lib
    assert _lib.get().idp is False
    s = m.Solver(name="o", gridSize=m.vec3(12, 10, 8), dim=3)
    _refused(m, _objects(m, s), r"the 'oracle' backend does not implement implicit density projection")


def test_z_slab_solver_refuses_the_plugins(oracle_backend):
    import manta as m
    s = m.Solver(name="o", gridSize=m.vec3(12, 10, 8), dim=3)
    o = _objects(m, s)
    s._slab_window = (4, 40)      # what slab.SlabDomain gives the solver of a z-slab: (z offset, global sz)
    try:
        _refused(m, o, r"implicit density projection does not run on a z-slab solver")
    finally:
        s._slab_window = (0, 0)


@pytest.mark.parametrize("dims", [(12, 10, 8), (15, 12, 1)])
def test_copy_flags_to_flags_on_the_cpu_backend(oracle_backend, dims):
    import manta as m
    s = m.Solver(name="o", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)
    a, b = s.create(m.FlagGrid), s.create(m.FlagGrid)
    src = np.random.RandomState(3).randint(0, 128, (dims[2], dims[1], dims[0])).astype(np.int32)
    a.from_numpy(src)
    m.copyFlagsToFlags(a, b)
    assert np.array_equal(b.to_numpy(), M.copy_flags(src)) and np.array_equal(a.to_numpy(), src)
    with pytest.raises(RuntimeError, match="can't convert argument to FlagGrid"):
        m.copyFlagsToFlags(a, s.create(m.IntGrid))


def _calls_outside_resampling(tree):
    """every ast.Call of the module, except inside an `if (resampleParticles)` body"""
    out = []

    def visit(node):
        if isinstance(node, ast.If) and isinstance(node.test, ast.Name) and node.test.id == "resampleParticles":
            for n in node.orelse:
                visit(n)
            return
        if isinstance(node, ast.Call):
            out.append(node)
        for ch in ast.iter_child_nodes(node):
            visit(ch)
    visit(tree)
    return out


@pytest.mark.parametrize("scene", ["idp_apic01_simple.py", "idp_apic02_3d.py"])
def test_scene_calls_bind(scene):
    """every call of a package-level name in the IDP scenes (outside the resampling branch, which is out of scope) binds against
    the package's signature; without the reference's scenes there is nothing to check"""
    path = os.path.join(SCENES, scene)
    if not os.path.exists(path):
        return
    import manta as m
    checked = set()
    for call in _calls_outside_resampling(ast.parse(open(path).read())):
        if not isinstance(call.func, ast.Name):
            continue
        name = call.func.id
        if name in ("range", "vec3", "mantaMsg", "Gui"):
            continue
        fn = getattr(m, name)      # a missing name is the failure this test exists for
        if inspect.isclass(fn):
            continue
        sig = inspect.signature(fn)
        args = [object()] * len(call.args)
        kw = {k.arg: object() for k in call.keywords}
        sig.bind(*args, **kw)
        checked.add(name)
    assert {"copyFlagsToFlags", "mapMassToGrid", "computeDeltaX", "mapMACToPartPositions", "solvePressureSystem", "apicMapPartsToMAC",
            "extrapolateMACSimple"} <= checked


def test_adapt_timestep_takes_cfl_as_a_real(oracle_backend):
    """FluidSolver::adaptTimestep, fluidsolver.cpp:186-189: mCflCond is a Real, so `mCflCond / (mvt + 1e-05)` divides the fp32 value of
    cfl (as a double) -- for a cfl that fp32 does not hold exactly (the recorded loops' 0.1) the step differs in the last bit from
    the one computed with the Python float"""
    import manta as m
    f32 = np.float32
    differ = 0
    for mv in np.linspace(0.12, 0.2, 400):
        s = m.Solver(name="o", gridSize=m.vec3(8, 8, 8), dim=3)
        s.frameLength, s.timestepMin, s.timestepMax, s.cfl = 10000000.0, 0.01, 1.0, 0.1
        s.timestep = 0.7695308
        s.adaptTimestep(float(f32(mv)))
        mvt = f32(mv) * f32(0.7695308)
        want = f32(f32(0.7695308) * f32(float(f32(0.1)) / (float(mvt) + 1e-05)))
        assert f32(s.timestep) == want, mv
        differ += want != f32(f32(0.7695308) * f32(0.1 / (float(mvt) + 1e-05)))
    assert differ >= 10
