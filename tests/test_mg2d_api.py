"""The 2-D multigrid preconditioner's public surface without a GPU: include/open/manta_hip_mg2d.h parses, its row is in the open
extension table and its entry names are its own, the HIP library (where built) exports it; the switch of mantaflow_amd.multigrid2d
is off after import and setMultigrid2D returns the previous value; with the switch off a 2-D solver gets today's refusal word for
word; with the switch on the CPU checker backend refuses by the extension's name with all grids unchanged, and a z-slab window is
refused as before; tests/golden/mg2d.npz stays a small, complete fixture."""
import ctypes
import glob
import os

import numpy as np
import pytest

import cases
import mg2d_cases as C
import util
from mg2d_cases import PcMGDynamic, PcMGStatic, PcMIC

ENTRIES = {"mf_mg2d_abi_version", "mf_mg2d_create", "mf_mg2d_destroy", "mf_mg2d_set_a", "mf_mg2d_is_a_set", "mf_mg2d_vcycle", "mf_mg2d_cg_solve",
           "mf_mg2d_info", "mf_mg2d_read_level"}
OLD_2D_MESSAGE = "%s: the multigrid preconditioners PcMGStatic / PcMGDynamic run on 3-D solvers only"


@pytest.fixture
def switch_on():
    """turns the process-wide switch on for one test and puts back what was there"""
    from mantaflow_amd import multigrid2d
    prev = multigrid2d.setMultigrid2D(True)
    try:
        yield
    finally:
        multigrid2d.setMultigrid2D(prev)


def test_header_parses_and_row_is_found():
    from mantaflow_amd import _lib
    row = _lib.extension("mg2d")
    assert row in _lib.OPEN_EXTENSIONS and row.header == _lib.MG2D_HEADER
    assert os.path.samefile(os.path.dirname(row.header), os.path.join(C.ROOT, "include", "open"))
    assert row.version_fn == "mf_mg2d_abi_version" and row.version_macro == "MF_MG2D_ABI_VERSION"
    protos = _lib.parse_header(row.header)
    assert set(protos) == ENTRIES
    # one for one with the 3-D entries, without sz and Ak
    three = _lib.parse_header(_lib.MULTIGRID_HEADER)
    assert {n.replace("mf_mg2d_", "mf_mg_").replace("mf_mg_abi_version", "mf_multigrid_abi_version") for n in protos} == set(three)
    assert len(protos["mf_mg2d_create"][1]) == 3 and protos["mf_mg2d_create"][1][2] is ctypes.c_void_p
    assert len(protos["mf_mg2d_set_a"][1]) == len(three["mf_mg_set_a"][1]) - 1
    assert len(protos["mf_mg2d_cg_solve"][1]) == len(three["mf_mg_cg_solve"][1]) - 2 == 17
    for name in ("vcycle", "info", "read_level", "destroy", "is_a_set"):
        assert protos["mf_mg2d_" + name] == three["mf_mg_" + name]
    # the names are this header's alone, and the headers under include/open/ are exactly the rows' headers
    for other in _lib.all_extensions():
        if other is not row:
            assert not (set(_lib.parse_header(other.header)) & ENTRIES), other.name
    assert not (set(_lib.parse_header()) & ENTRIES)
    assert sorted(glob.glob(os.path.join(C.ROOT, "include", "open", "manta_hip_*.h"))) == sorted(e.header for e in _lib.OPEN_EXTENSIONS)
    text = open(row.header).read()
    assert "multigrid.cpp:" in text and "conjugategrad.cpp:" in text
    if os.path.exists(util.HIP_LIB):
        L = ctypes.CDLL(util.HIP_LIB)
        for name in protos:
            assert hasattr(L, name), name
        assert L.mf_mg2d_abi_version() == 1


def test_switch_is_off_after_import_and_returns_previous_value():
    from mantaflow_amd import api, multigrid2d, plugins
    import manta
    assert multigrid2d.multigrid2DEnabled() is False and plugins._multigrid_2d is False
    assert not hasattr(api, "setMultigrid2D") and not hasattr(manta, "setMultigrid2D") and not hasattr(manta, "multigrid2DEnabled")
    try:
        assert multigrid2d.setMultigrid2D() is False
        assert multigrid2d.multigrid2DEnabled() is True
        assert multigrid2d.setMultigrid2D(True) is True
        assert multigrid2d.setMultigrid2D(False) is True
        assert multigrid2d.multigrid2DEnabled() is False
        assert multigrid2d.setMultigrid2D(0) is False and multigrid2d.multigrid2DEnabled() is False
    finally:
        multigrid2d.setMultigrid2D(False)


def test_module_is_the_first_import_of_a_scene():
    """the two opt-in lines stand in front of a scene: the module must import before anything else of the package was imported,
    and importing it must not flip the switch (a fresh interpreter: in this one the package is long imported)"""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from mantaflow_amd.multigrid2d import setMultigrid2D, multigrid2DEnabled\n"
            "from mantaflow_amd import plugins\n"
            "assert multigrid2DEnabled() is False and plugins._multigrid_2d is False\n"
            "assert setMultigrid2D() is False and plugins._multigrid_2d is True\n"
            "print('ok')\n") % C.ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def _solver_2d(dims=(24, 20, 1)):
    from mantaflow_amd import core
    s = cases._mk_solver(dims)
    fl, v, p, rhs = core.FlagGrid(s), core.MACGrid(s), core.Grid(s), core.Grid(s)
    flags = util.make_flags(*dims, seed=1)
    vel = util.smooth_vel(*dims, 1)
    cases.soa_to_grid(fl, flags); cases.soa_to_grid(v, vel)
    p.setConst(3.0); rhs.setConst(2.0)
    return s, fl, v, p, rhs, vel


def _assert_untouched(v, p, rhs, vel):
    assert (cases.grid_to_soa(p) == 3.0).all() and (cases.grid_to_soa(rhs) == 2.0).all()
    util.assert_bitexact(cases.grid_to_soa(v), vel, "vel untouched")


class _FakeLib(object):
    """what _multigrid_lib looks at, for the decisions no library on this machine leads to"""
    path = "libfake.so"

    def __init__(self, backend, multigrid, mg2d):
        self.backend, self.multigrid, self.mg2d = backend, multigrid, mg2d


class _FakeSolver(object):
    def __init__(self, lib, three_d, window=(0, 0)):
        self.lib, self._three_d, self._slab_window = lib, three_d, window

    def is3D(self):
        return self._three_d


@pytest.mark.parametrize("pc", [PcMGStatic, PcMGDynamic])
def test_switch_off_keeps_todays_messages(oracle_backend, pc):
    """on the checker backend the extension's refusal comes first, as it always did; the 2-D message is today's, word for word"""
    from mantaflow_amd import multigrid2d, plugins
    assert multigrid2d.multigrid2DEnabled() is False
    s, fl, v, p, rhs, vel = _solver_2d()
    with pytest.raises(RuntimeError, match=r"^solvePressure: the 'oracle' backend does not implement the multigrid preconditioners PcMGStatic / PcMGDynamic \(manta_hip_multigrid.h\)$"):
        plugins.solvePressure(v, p, fl, preconditioner=pc)
    _assert_untouched(v, p, rhs, vel)
    for name in ("solvePressure", "solvePressureSystem", "PD_fluid_guiding"):
        with pytest.raises(RuntimeError) as e:
            plugins._multigrid_lib(_FakeSolver(_FakeLib("hip", True, True), False), name)
        assert str(e.value) == OLD_2D_MESSAGE % name
    assert plugins._multigrid_lib(_FakeSolver(_FakeLib("hip", True, False), True), "solvePressure").backend == "hip"      # 3-D: as ever


@pytest.mark.parametrize("pc", [PcMGStatic, PcMGDynamic])
def test_switch_on_checker_backend_refuses_by_name(oracle_backend, switch_on, pc):
    from mantaflow_amd import core, plugins
    s, fl, v, p, rhs, vel = _solver_2d()
    assert s.lib.mg2d is False
    what = r"the 'oracle' backend does not implement the multigrid preconditioners PcMGStatic / PcMGDynamic on 2-D solvers \(manta_hip_mg2d.h\)$"
    with pytest.raises(RuntimeError, match=r"^solvePressure: " + what):
        plugins.solvePressure(v, p, fl, preconditioner=pc, zeroPressureFixing=True)
    with pytest.raises(RuntimeError, match=r"^solvePressureSystem: " + what):
        plugins.solvePressureSystem(rhs, v, p, fl, preconditioner=pc)
    _assert_untouched(v, p, rhs, vel)
    assert s._mg is None
    plugins.releaseMG(s)
    # a 3-D solver is not the switch's business
    s3 = cases._mk_solver((12, 10, 8))
    with pytest.raises(RuntimeError, match=r"\(manta_hip_multigrid.h\)$"):
        plugins.solvePressure(core.MACGrid(s3), core.Grid(s3), core.FlagGrid(s3), preconditioner=pc)
    # PcMIC on the same 2-D inputs still solves (plain CG with the x4 cap)
    plugins.solvePressure(v, p, fl, preconditioner=PcMIC, zeroPressureFixing=True)
    assert 0 < plugins.lastCgStats()["iterations"] and not (cases.grid_to_soa(p) == 3.0).all()


def test_switch_on_gate_decisions(switch_on):
    from mantaflow_amd import plugins
    gate = plugins._multigrid_lib
    lib = _FakeLib("hip", True, True)
    assert gate(_FakeSolver(lib, False), "solvePressure") is lib
    assert gate(_FakeSolver(lib, True), "solvePressure") is lib
    with pytest.raises(RuntimeError) as e:
        gate(_FakeSolver(_FakeLib("hip", True, False), False), "solvePressureSystem")
    assert str(e.value) == "solvePressureSystem: libfake.so lacks the 2-D multigrid extension (manta_hip_mg2d.h) -- rebuild the library"
    with pytest.raises(RuntimeError) as e:
        gate(_FakeSolver(lib, False, window=(4, 40)), "solvePressure")
    assert str(e.value) == "solvePressure: the multigrid preconditioners PcMGStatic / PcMGDynamic on 2-D solvers do not run on a z-slab solver"


def test_slab_window_is_refused_as_today(oracle_backend, switch_on):
    from mantaflow_amd import core, plugins
    s = cases._mk_solver((24, 20, 16))
    s._slab_window = (4, 40)
    fl, v, p = core.FlagGrid(s), core.MACGrid(s), core.Grid(s)
    p.setConst(3.0)
    with pytest.raises(RuntimeError, match=r"^solvePressure: the multigrid preconditioners PcMGStatic / PcMGDynamic do not run on a z-slab solver$"):
        plugins.solvePressure(v, p, fl, preconditioner=PcMGStatic)
    s._slab_window = (0, 0)
    assert (cases.grid_to_soa(p) == 3.0).all()


def test_handle_picks_the_2d_entries():
    from mantaflow_amd import plugins
    calls = []

    class Lib(object):
        def call(self, name, *args):
            calls.append((name, len(args)))

    h = plugins._MgHandle(Lib(), 24, 20, 1)
    keys = set(h.info())
    h.release()
    h3 = plugins._MgHandle(Lib(), 24, 20, 8)
    h3.release()
    assert [c[0] for c in calls] == ["mf_mg2d_create", "mf_mg2d_info", "mf_mg2d_destroy", "mf_mg_create", "mf_mg_destroy"]
    assert calls[0][1] == 3 and calls[3][1] == 4
    assert keys == {"levels", "setups", "coarse_cg_iterations", "nonzero_stencil_sum", "trivial_equations", "tail_first_level", "setup_host_us",
                    "setup_device_us", "sizes", "active"}      # info() keeps its keys


def test_golden_file_is_small_and_complete():
    assert os.path.getsize(C.GOLDEN) < (1 << 20)
    g = np.load(C.GOLDEN)
    assert len(C.CASES) == 4 * len(C.SHAPES) - len(C.EXCLUDED) and all(n.split("_")[1] in ("3x400x1", "400x3x1") for n in C.EXCLUDED)
    for kind, dims in C.CASES:
        name = C.case_name(kind, dims)
        assert 0 < int(g[name + "__iters"]) < 100 and g[name + "__sha_p"].shape == (32,) and g[name + "__sha_v"].shape == (32,)
    for name in C.EXCLUDED:
        assert name + "__iters" not in g.files
    assert 0 < int(g[C.FRACTIONS_NAME + "__iters"]) < 100
    for tag in C.stage_tags():
        nl = int(g[tag + "__levels"])
        assert [tuple(int(v) for v in g[tag + "__size%d" % l]) for l in range(nl)] == (C.LEVELS.get(C.stage_system_dims(tag)) or C.FRACTIONS_LEVELS)
    assert (g["plume/cg"] < 100).all() and (g["guiding/cg"] < 100).all() and (g["flip/cg"] < 100).all() and (g["guiding/pd"] < 200).all()
    assert len(g["plume/cg"]) == C.PLUME["steps"] and len(g["guiding/pd"]) == C.GUIDING["steps"] and len(g["flip/cg"]) == C.FLIP["steps"]
    assert len(g["guiding/cg"]) == int(g["guiding/pd"].sum()) + C.GUIDING["steps"]
    for k in g.files:
        assert g[k].size <= 4096, k      # larger arrays are digests
