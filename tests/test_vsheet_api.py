"""CPU: the public face of vortex sheets without a GPU -- the opt-in module and its names with the reference's signatures, their absence
from `manta`, the row of the open extension table with its header, entry names disjoint from every other extension, the refusals by name
(the CPU checker backend, a z-slab solver) with mesh, channels and process state left as they were, the channel defaults after each
rebuilding route and the length-mismatch error (through the channel bookkeeping, which needs no kernel), and resetVortexSheetState.
The 2-D refusal and the argument checks come after those refusals and are checked in tests/test_gpu_vsheet.py with the kernels."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest

import meshops_model as MO
import util
import vsheet_model as M

f32 = np.float32
PLUGINS = ("VICintegration", "smoothVorticity", "vorticitySource", "texcoordInflow", "meshSmokeInflow")
NAMES = ("VortexSheetMesh",) + PLUGINS + ("resetVortexSheetState", "lastVortexSheetStats")


def test_names_are_opt_in_and_signatures():
    import manta
    from mantaflow_amd import api, core, vortexsheet as vs
    assert set(NAMES) <= set(vs.__all__)
    for n in NAMES:
        assert not hasattr(manta, n) and not hasattr(api, n), n
    assert issubclass(vs.VortexSheetMesh, core.Mesh)
    assert str(inspect.signature(vs.VICintegration)) == (
        "(mesh, sigma, vel, flags, vorticity=None, cgMaxIterFac=1.5, cgAccuracy=0.001, scale=0.01, precondition=0)")
    assert str(inspect.signature(vs.smoothVorticity)) == "(mesh, iter=1, sigma=0.2, alpha=0.8)"
    assert str(inspect.signature(vs.vorticitySource)) == "(mesh, gravity, vel=None, velOld=None, scale=0.1, maxAmount=0, mult=1.0)"
    assert str(inspect.signature(vs.texcoordInflow)) == "(mesh, shape, vel)"
    assert str(inspect.signature(vs.meshSmokeInflow)) == "(mesh, shape, amount)"
    assert str(inspect.signature(vs.resetVortexSheetState)) == "()"
    assert str(inspect.signature(vs.lastVortexSheetStats)) == "()" and isinstance(vs.lastVortexSheetStats(), dict)
    for meth in ("calcVorticity", "calcCirculation", "reinitTexCoords", "sheet_numpy", "tex_numpy", "turb_numpy"):
        assert str(inspect.signature(getattr(vs.VortexSheetMesh, meth))) == "(self)", meth
    assert str(inspect.signature(vs.VortexSheetMesh.set_sheet_numpy)) == (
        "(self, vorticity=None, vorticitySmoothed=None, circulation=None, smokeAmount=None, smokeParticles=None)")
    assert str(inspect.signature(vs.VortexSheetMesh.set_tex_numpy)) == "(self, tex1=None, tex2=None)"
    g = {}
    exec("from mantaflow_amd.vortexsheet import *\nfrom manta import *", g)       # how a scene gets the family
    assert g["VortexSheetMesh"] is vs.VortexSheetMesh and g["vorticitySource"] is vs.vorticitySource and "Solver" in g
    import manta as again
    for n in NAMES:
        assert not hasattr(again, n), n


def test_row_of_the_open_table_and_header():
    from mantaflow_amd import _lib
    e = _lib.extension("vsheet")
    assert e in _lib.OPEN_EXTENSIONS and (e.what, e.verb) == ("vortex sheets", "do")
    inc = os.path.dirname(_lib.HEADER)
    assert e.header == os.path.join(inc, "open", "manta_hip_vsheet.h") == _lib.VSHEET_HEADER and os.path.exists(e.header)
    assert {x.header for x in _lib.OPEN_EXTENSIONS} == set(glob.glob(os.path.join(inc, "open", "manta_hip_*.h")))
    assert (e.version_fn, e.version_macro) == ("mf_vsheet_abi_version", "MF_VSHEET_ABI_VERSION")
    assert re.search(r"^#define\s+MF_VSHEET_ABI_VERSION\s+\d+\s*$", open(e.header).read(), flags=re.M)
    restype, argtypes, _ = _lib.parse_header(e.header)[e.version_fn]
    assert restype is ctypes.c_int and argtypes == []


def test_entry_names_are_disjoint_and_every_entry_cites_the_reference():
    from mantaflow_amd import _lib
    seen = {n: "manta_hip.h" for n in _lib.parse_header()}
    for e in _lib.all_extensions():
        if e.name != "vsheet":
            for n in _lib.parse_header(e.header):
                seen[n] = os.path.basename(e.header)
    mine = _lib.parse_header(_lib.VSHEET_HEADER)
    assert mine and all(n.startswith("mf_vsheet_") for n in mine)
    for n in mine:
        assert n not in seen, "%s is declared by %s as well" % (n, seen.get(n))
    text = open(_lib.VSHEET_HEADER).read()
    for n in mine:
        if n == "mf_vsheet_abi_version":
            continue
        comment = text[:text.index("int " + n + "(")].rsplit("/*", 1)[1]
        assert re.search(r"(vortexsheet|vortexplugins)\.cpp:\d+", comment), n


@pytest.mark.skipif(not os.path.exists(util.HIP_LIB), reason="libmanta_hip.so not built")
def test_the_product_library_exports_the_extension():
    from mantaflow_amd import _lib
    L = ctypes.CDLL(util.HIP_LIB)          # loads without a GPU
    for n in _lib.parse_header(_lib.VSHEET_HEADER):
        assert hasattr(L, n), n
    assert L.mf_vsheet_abi_version() == 1


def _scene(m, vs):
    s = m.Solver(name="o", gridSize=m.vec3(*M.DIMS), dim=3)
    mesh = s.create(vs.VortexSheetMesh)
    model = MO.bipyramid(5, centre=(6.0, 6.0, 6.0))
    mesh.set_numpy(model["pos"], None, model["flags"], model["tris"], None)
    return s, mesh, model


def _snapshot(mesh, vs):
    pos, normal, fl = mesh.nodes_numpy()
    tris, tfl = mesh.tris_numpy()
    return [pos.tobytes(), fl.tobytes(), tris.tobytes(), mesh._topo_gen, mesh._ch_fresh, mesh._ch_nt, mesh._ch_nn, sorted(mesh._ch), mesh.mTexOffset,
            vs._state.t0, vs.lastVortexSheetStats()]


def test_refusals_name_the_caller_and_touch_nothing(oracle_backend):
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    vs.resetVortexSheetState()
    s, mesh, _ = _scene(m, vs)
    vel, old = s.create(m.MACGrid), s.create(m.MACGrid)
    box = m.Box(parent=s, p0=m.vec3(1, 1, 1), p1=m.vec3(5, 5, 5))
    before = _snapshot(mesh, vs)
    calls = {"meshSmokeInflow": lambda: vs.meshSmokeInflow(mesh, box, 0.5), "texcoordInflow": lambda: vs.texcoordInflow(mesh, box, vel),
             "smoothVorticity": lambda: vs.smoothVorticity(mesh), "vorticitySource": lambda: vs.vorticitySource(mesh, m.vec3(0, -1, 0), vel, old),
             "VICintegration": lambda: vs.VICintegration(mesh, 1.5, vel, s.create(m.FlagGrid), precondition=2),
             "bad arguments": lambda: vs.vorticitySource(mesh, "gravity", 3, 4)}
    for meth in ("calcVorticity", "reinitTexCoords", "sheet_numpy", "tex_numpy", "turb_numpy", "set_sheet_numpy", "set_tex_numpy"):
        calls["VortexSheetMesh::" + meth] = getattr(mesh, meth)
    for who, call in calls.items():
        who = "vorticitySource" if who == "bad arguments" else who          # refused by name before the arguments are looked at
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == who + ": the 'oracle' backend does not implement vortex sheets (manta_hip_vsheet.h)"
    s._slab_window = (2, 8)
    try:
        for who, call in calls.items():
            who = "vorticitySource" if who == "bad arguments" else who
            with pytest.raises(RuntimeError) as e:
                call()
            assert str(e.value) == who + ": vortex sheets do not run on a z-slab solver"
    finally:
        s._slab_window = (0, 0)
    with pytest.raises(RuntimeError) as e:
        mesh.calcCirculation()
    assert str(e.value).startswith("VortexSheetMesh::calcCirculation: not implemented in mantaflow_amd (")
    assert _snapshot(mesh, vs) == before


def test_a_plain_mesh_keeps_its_refusals_and_a_sheet_is_a_mesh(oracle_backend):
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    s, mesh, model = _scene(m, vs)
    plain = s.create(m.Mesh)
    for obj in (plain, mesh):
        for name, call in (("fromShape", obj.fromShape), ("computeVelocity", obj.computeVelocity), ("create", obj.create),
                           ("getNodesDataPointer", obj.getNodesDataPointer), ("getTrisDataPointer", obj.getTrisDataPointer)):
            with pytest.raises(RuntimeError, match=r"^Mesh::%s: not implemented in mantaflow_amd \(" % name):
                call()
    assert not hasattr(plain, "calcVorticity") and not hasattr(plain, "sheet_numpy")
    assert mesh.numTris() == model["tris"].shape[0] and np.array_equal(mesh.tris_numpy()[0], model["tris"])
    with pytest.raises(RuntimeError, match="can't convert argument to PbType"):
        s.create("VortexSheetMesh")


def _channel_rows(mesh):
    from mantaflow_amd import vortexsheet as vs
    out = {}
    for table, cap, n in ((vs._TRI_CHANNELS, mesh.tcap, mesh.nt), (vs._NODE_CHANNELS, mesh.ncap, mesh.nn)):
        for key, ncomp, _ in table:
            out[key] = mesh._ch[key].view(ncomp, cap)[:, :n].cpu().numpy().copy()
    return out


def _dirty(mesh):
    for t in mesh._ch.values():
        t.fill_(7.5)


def test_channel_defaults_after_every_rebuilding_route_and_the_length_mismatch(oracle_backend, tmp_path):
    """the bookkeeping behind every sheet call (VortexSheetMesh._channels), which needs no kernel: defaults on the first use after
    set_numpy / load / clear, nothing reset in between, and the refusal once the counts have moved without the channels"""
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    s, mesh, model = _scene(m, vs)
    path = str(tmp_path / "sheet.bobj.gz")
    mesh.save(path)

    def defaults():
        rows = _channel_rows(mesh)
        assert set(rows) == {"vorticity", "vorticitySmoothed", "circulation", "smokeAmount", "smokeParticles", "tex1", "tex2", "turb"}
        for k, a in rows.items():
            assert a.shape[1] == (mesh.nt if k in M.DEFAULTS else mesh.nn)
            assert (a == f32(M.DEFAULTS.get(k, 0.0))).all(), k

    routes = (("set_numpy", lambda: mesh.set_numpy(model["pos"], None, model["flags"], model["tris"], None)), ("load", lambda: mesh.load(path)),
              ("clear", mesh.clear), ("larger", lambda: mesh.set_numpy(*[MO.bipyramid(40)[k] for k in ("pos", "normal", "flags", "tris", "tflags")])))
    mesh._channels("calcVorticity")
    defaults()
    for name, route in routes:
        _dirty(mesh)
        route()
        assert mesh._channels("calcVorticity") is mesh._ch
        defaults()
        _dirty(mesh)
        mesh._channels("calcVorticity")          # a second use resets nothing
        assert all((a == f32(7.5)).all() for a in _channel_rows(mesh).values()), name
    # a route that does not know the channels: the counts move, the channels keep their length
    mesh.nt -= 2
    mesh._topo_gen += 1
    for who in ("calcVorticity", "sheet_numpy"):
        with pytest.raises(RuntimeError) as e:
            mesh._channels(who)
        assert str(e.value) == "VortexSheetMesh::%s: channels do not match the mesh (78 triangles and 42 nodes, channels of 80 and 42)" % who
    mesh.clear()                                 # a rebuilding route puts it right
    mesh._channels("calcVorticity")
    assert (mesh._ch_nt, mesh._ch_nn) == (0, 0)


def test_reset_state_puts_the_offset_back():
    from mantaflow_amd import vortexsheet as vs
    vs._state.t0 = (1.0, 2.0, 3.0)
    vs._stats["source"] = dict(max=1.0, mean=0.5)
    assert vs.lastVortexSheetStats() == {"source": {"max": 1.0, "mean": 0.5}}
    vs.resetVortexSheetState()
    assert vs._state.t0 == (0.0, 0.0, 0.0) and vs.lastVortexSheetStats() == {}
