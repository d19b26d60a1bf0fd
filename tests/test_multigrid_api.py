"""The multigrid preconditioner's public surface without a GPU: releaseMG is exported, include/manta_hip_multigrid.h parses and the HIP
library (where built) exports it, the CPU checker backend refuses PcMGStatic / PcMGDynamic by name and leaves the grids alone, and
tests/golden/multigrid.npz (described at the top of tests/test_gpu_multigrid.py) stays a small fixture."""
import ctypes
import os

import numpy as np
import pytest

import cases
import mg_cases
import util
from mg_cases import PcMGDynamic, PcMGStatic, PcMIC


def test_release_mg_is_exported():
    ns = {}
    exec("from manta import *", ns)
    assert callable(ns["releaseMG"]) and ns["PcMGDynamic"] == 2 and ns["PcMGStatic"] == 3
    from mantaflow_amd import api
    assert api.releaseMG is ns["releaseMG"]


def test_header_parses_and_library_exports_it():
    from mantaflow_amd import _lib
    protos = _lib.parse_header(_lib.MULTIGRID_HEADER)
    want = {"mf_multigrid_abi_version", "mf_mg_create", "mf_mg_destroy", "mf_mg_set_a", "mf_mg_is_a_set", "mf_mg_vcycle", "mf_mg_cg_solve",
            "mf_mg_info", "mf_mg_read_level"}
    assert set(protos) == want
    assert len(protos["mf_mg_cg_solve"][1]) == 19 and protos["mf_mg_create"][1][3] is ctypes.c_void_p
    # the frozen core header knows nothing of it
    assert not (set(_lib.parse_header()) & want)
    if os.path.exists(util.HIP_LIB):
        L = ctypes.CDLL(util.HIP_LIB)
        for name in protos:
            assert hasattr(L, name), name
        assert L.mf_multigrid_abi_version() == 1


@pytest.mark.parametrize("pc", [PcMGStatic, PcMGDynamic])
def test_oracle_backend_refuses_by_name(oracle_backend, pc):
    from mantaflow_amd import core, plugins
    dims = (16, 12, 10)
    flags, vel, phi, kw = mg_cases.inputs("obs", dims)
    s = cases._mk_solver(dims)
    assert s.lib.multigrid is False
    fl, v, p = core.FlagGrid(s), core.MACGrid(s), core.Grid(s)
    cases.soa_to_grid(fl, flags); cases.soa_to_grid(v, vel)
    p.setConst(3.0)
    with pytest.raises(RuntimeError, match=r"solvePressure: the 'oracle' backend does not implement the multigrid preconditioners PcMGStatic / PcMGDynamic"):
        plugins.solvePressure(v, p, fl, preconditioner=pc, **kw)
    rhs = core.Grid(s)
    with pytest.raises(RuntimeError, match=r"solvePressureSystem: the 'oracle' backend does not implement the multigrid"):
        plugins.solvePressureSystem(rhs, v, p, fl, preconditioner=pc, **kw)
    assert (cases.grid_to_soa(p) == 3.0).all()
    util.assert_bitexact(cases.grid_to_soa(v), vel, "vel untouched")
    plugins.releaseMG(s)      # nothing to release: no error
    plugins.releaseMG()
    # PcMIC on the same inputs still solves
    plugins.solvePressure(v, p, fl, preconditioner=PcMIC, **kw)
    assert 0 < plugins.lastCgStats()["iterations"] < 100 and np.abs(cases.grid_to_soa(p)).max() > 0 and not (cases.grid_to_soa(p) == 3.0).any()


def test_golden_file_is_small_and_complete():
    assert os.path.getsize(mg_cases.GOLDEN) < (1 << 20)
    g = np.load(mg_cases.GOLDEN)
    for kind in mg_cases.KINDS:
        for dims in mg_cases.SIZES:
            assert 0 < int(g["iters__" + mg_cases.case_name(kind, dims)]) < 100
    for kind, dims in mg_cases.STAGE_CASES.items():
        name = mg_cases.case_name(kind, dims)
        nl = int(g["stage__%s__levels" % name])
        assert nl == 3 and g["stage__%s__A1" % name].shape[0] == 14 and ("stage__%s__A%d" % (name, nl - 1)) in g.files
    for tag in ["static__a", "static__b", "static__c"] + ["mgsolve__%d" % i for i in range(4)]:
        assert 0 < int(g[tag + "__iters"]) < 100 and g[tag + "__sha_p"].shape == (32,)
    assert int(g["fractions__0.0001__iters"]) == 5 and int(g["fractions__0.001__iters"]) == 4
