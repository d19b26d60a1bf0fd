"""The z-slab multigrid preconditioner's public surface without a GPU: include/open/manta_hip_mgslab.h parses, its row is in the
open extension table, its entry names are its own and the HIP library (where built) exports them; slab.solvePressure refuses --
by name, before it touches a grid and before any collective -- a preconditioner value that is none of the three, the CPU checker
backend (which has no multigrid) and a HIP library without the extension; preconditioner=PcMIC is today's solve, bit for bit;
slab.releaseMG / applyMG on a domain without a hierarchy; the coarse-plane ownership rule of slab.py is the model's."""
import ctypes
import glob
import os

import numpy as np
import pytest

import cases
import mgslab_model
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mf_mgslab_abi_version", "mf_mgslab_set_accuracy", "mf_mgslab_set_rhs", "mf_mgslab_smooth", "mf_mgslab_residual",
           "mf_mgslab_restrict", "mf_mgslab_coarse", "mf_mgslab_interp_add", "mf_mgslab_get_planes", "mf_mgslab_put_planes"}
DIMS = (20, 16, 12)


def test_header_parses_and_row_is_found():
    from mantaflow_amd import _lib
    row = _lib.extension("mgslab")
    assert row in _lib.OPEN_EXTENSIONS and row.header == _lib.MGSLAB_HEADER
    assert os.path.samefile(os.path.dirname(row.header), os.path.join(ROOT, "include", "open"))
    assert row.version_fn == "mf_mgslab_abi_version" and row.version_macro == "MF_MGSLAB_ABI_VERSION"
    protos = _lib.parse_header(row.header)
    assert set(protos) == ENTRIES
    # every entry but the revision takes the handle of mf_mg_create first; the ranged ones end with the stream
    for name, (restype, argtypes, argnames) in protos.items():
        if name != "mf_mgslab_abi_version":
            assert argtypes[0] is ctypes.c_void_p and argnames[0] == "handle", name
        if name not in ("mf_mgslab_abi_version", "mf_mgslab_set_accuracy"):
            assert argnames[-1] == "stream", name
    # the names are this header's alone, and the headers under include/open/ are exactly the rows' headers
    for other in _lib.all_extensions():
        if other is not row:
            assert not (set(_lib.parse_header(other.header)) & ENTRIES), other.name
    assert not (set(_lib.parse_header()) & ENTRIES)
    assert sorted(glob.glob(os.path.join(ROOT, "include", "open", "manta_hip_*.h"))) == sorted(e.header for e in _lib.OPEN_EXTENSIONS)
    text = open(row.header).read()
    assert "multigrid.cpp:" in text and "conjugategrad.cpp:" in text
    if os.path.exists(util.HIP_LIB):
        L = ctypes.CDLL(util.HIP_LIB)
        for name in protos:
            assert hasattr(L, name), name
        assert L.mf_mgslab_abi_version() == 1


def test_frozen_headers_keep_their_revisions():
    from mantaflow_amd import _lib
    assert "#define MF_MULTIGRID_ABI_VERSION 1" in open(_lib.MULTIGRID_HEADER).read()
    assert "mgslab" not in open(_lib.MULTIGRID_HEADER).read() and "mgslab" not in open(_lib.HEADER).read()


def _slab_inputs():
    from mantaflow_amd import core, slab
    dom = slab.SlabDomain(DIMS, 2)
    s = dom.solver
    flags_g = util.make_flags(*DIMS, 51, obstacles=True, empty_top=True)
    vel_g = util.smooth_vel(*DIMS, 52, 2.0)
    flags, vel, pres = core.FlagGrid(s), core.MACGrid(s), core.Grid(s)
    dom.scatter_global(flags, flags_g); dom.scatter_global(vel, vel_g)
    slab.setWallBcs(dom, flags, vel)
    pres.setConst(3.0)
    return dom, flags, vel, pres


class _NoCollective(object):
    """a communicator on which every collective is an error"""
    world, rank, on = 1, 0, False

    def __getattr__(self, name):
        raise AssertionError("collective %s reached before the refusal" % name)


def _refused(dom, flags, vel, pres, pc, message):
    from mantaflow_amd import slab
    vel0, flags0 = cases.grid_to_soa(vel), cases.grid_to_soa(flags)
    comm, dom.comm = dom.comm, _NoCollective()
    try:
        with pytest.raises(RuntimeError) as e:
            slab.solvePressure(dom, vel, pres, flags, preconditioner=pc)
    finally:
        dom.comm = comm
    assert str(e.value) == message
    util.assert_bitexact(cases.grid_to_soa(vel), vel0, "vel untouched")
    assert (cases.grid_to_soa(flags) == flags0).all() and (cases.grid_to_soa(pres) == 3.0).all()
    assert getattr(dom, "_mg", None) is None


@pytest.mark.parametrize("pc", [0, 4, -1, "PcMGStatic", None, True, 2.5])
def test_unknown_preconditioner_is_refused_by_name(oracle_backend, pc):
    dom, flags, vel, pres = _slab_inputs()
    _refused(dom, flags, vel, pres, pc,
             "slab.solvePressure: preconditioner must be PcMIC (1), PcMGDynamic (2) or PcMGStatic (3), got %r" % (pc,))


@pytest.mark.parametrize("pc", [2, 3])
def test_checker_backend_is_refused_by_name(oracle_backend, pc):
    from mantaflow_amd import slab
    assert (slab.PcMIC, slab.PcMGDynamic, slab.PcMGStatic) == (1, 2, 3)
    dom, flags, vel, pres = _slab_inputs()
    assert dom.solver.lib.mgslab is False and dom.solver.lib.multigrid is False
    _refused(dom, flags, vel, pres, pc, "slab.solvePressure: the 'oracle' backend does not implement the multigrid preconditioners "
             "PcMGStatic / PcMGDynamic on z-slabs (manta_hip_mgslab.h)")


class _FakeLib(object):
    path = "libfake.so"

    def __init__(self, backend, multigrid, mgslab):
        self.backend, self.multigrid, self.mgslab = backend, multigrid, mgslab


class _FakeDom(object):
    def __init__(self, lib):
        self.solver = type("S", (), {"lib": lib})()


def test_gate_decisions():
    from mantaflow_amd import slab
    gate = slab._mg_wanted
    full = _FakeDom(_FakeLib("hip", True, True))
    assert gate(full, 1) is False and gate(full, 2) is True and gate(full, 3) is True
    # PcMIC asks nothing of the library
    assert gate(_FakeDom(_FakeLib("oracle", False, False)), 1) is False
    for lib in (_FakeLib("hip", True, False), _FakeLib("hip", False, False)):
        for pc in (2, 3):
            with pytest.raises(RuntimeError) as e:
                gate(_FakeDom(lib), pc)
            assert str(e.value) == "slab.solvePressure: libfake.so lacks the z-slab multigrid extension (manta_hip_mgslab.h) -- rebuild the library"
    # the value is looked at first, whatever the library
    with pytest.raises(RuntimeError, match=r"^slab.solvePressure: preconditioner must be"):
        gate(_FakeDom(_FakeLib("oracle", False, False)), 7)


def test_pcmic_is_todays_solve(oracle_backend):
    """the default and preconditioner=PcMIC: the same pressure, velocity, iteration count and stats keys, bit for bit"""
    from mantaflow_amd import slab
    out = []
    for kw in ({}, dict(preconditioner=slab.PcMIC), dict(preconditioner=1)):
        dom, flags, vel, pres = _slab_inputs()
        st = {}
        it = slab.solvePressure(dom, vel, pres, flags, cgAccuracy=1e-4, stats=st, **kw)
        assert it == st["iterations"] > 0 and set(st) == {"iterations", "residual", "mic_blocking"}
        assert getattr(dom, "_mg", None) is None
        out.append((it, cases.grid_to_soa(pres), cases.grid_to_soa(vel)))
    for it, p, v in out[1:]:
        assert it == out[0][0]
        util.assert_bitexact(p, out[0][1], "pressure")
        util.assert_bitexact(v, out[0][2], "velocity")


def test_release_and_apply_without_a_hierarchy(oracle_backend):
    from mantaflow_amd import core, slab
    dom, flags, vel, pres = _slab_inputs()
    slab.releaseMG(dom)
    slab.releaseMG(dom)
    assert dom._mg is None
    with pytest.raises(RuntimeError, match=r"^slab.applyMG: the domain holds no multigrid hierarchy"):
        slab.applyMG(dom, core.Grid(dom.solver), pres)
    assert (cases.grid_to_soa(pres) == 3.0).all()


def test_coarse_plane_rule_is_the_models():
    from mantaflow_amd import slab
    for NZ in range(2, 41):
        for z0 in range(NZ):
            for z1 in range(z0 + 1, NZ + 1):
                k0, k1 = slab.coarse_planes(z0, z1, NZ)
                assert (k0, k1) == mgslab_model.coarse_planes(z0, z1, NZ)
                want = [k for k in range((NZ + 2) // 2) if z0 <= min(2 * k, NZ - 1) < z1]
                assert list(range(k0, k1)) == want, (NZ, z0, z1)
