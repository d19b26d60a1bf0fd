"""The table of C ABI extensions (mantaflow_amd._lib.EXTENSIONS), without a GPU: the headers under include/ are exactly the ones the
table derives, each follows the naming rule (MF_<NAME>_ABI_VERSION, mf_<name>_abi_version), no two headers share a name, the CPU
checker backend has none of the extensions and SolverLib mirrors every flag, and one plugin of each extension refuses -- before
anything is touched -- a z-slab solver first and a backend without the extension second.  The refusal texts are written out here:
they are the contract, not the table's phrases."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

NAMES = ("obstacles", "multigrid", "resample", "idp", "partls", "guiding", "secparts")

# extension -> (plugin, the phrase of its refusals, the verb of the z-slab refusal)
REFUSALS = {
    "obstacles": ("updateFractions", "the fill-fraction obstacle plugins", "do"),
    "multigrid": ("solvePressure", "the multigrid preconditioners PcMGStatic / PcMGDynamic", "do"),
    "resample": ("combineGridVel", "particle resampling", "does"),
    "idp": ("computeDeltaX", "implicit density projection", "does"),
    "partls": ("averagedParticleLevelset", "the smooth particle level sets", "do"),
    "guiding": ("PD_fluid_guiding", "fluid guiding", "does"),
    "secparts": ("setMACFromLevelset", "the secondary particles", "do"),
}


def _backend_message(name):
    plugin, what, _ = REFUSALS[name]
    return "%s: the 'oracle' backend does not implement %s (manta_hip_%s.h)" % (plugin, what, name)


def _slab_message(name):
    plugin, what, verb = REFUSALS[name]
    return "%s: %s %s not run on a z-slab solver" % (plugin, what, verb)


def test_the_table_names_the_headers_of_the_tree():
    from mantaflow_amd import _lib
    assert tuple(e.name for e in _lib.EXTENSIONS) == NAMES
    inc = os.path.dirname(_lib.HEADER)
    assert {e.header for e in _lib.EXTENSIONS} == set(glob.glob(os.path.join(inc, "manta_hip_*.h")))
    for e in _lib.EXTENSIONS:
        assert e.header == os.path.join(inc, "manta_hip_%s.h" % e.name)
        assert getattr(_lib, e.name.upper() + "_HEADER") == e.header      # the names tests and tools import
        assert _lib.extension(e.name) is e


@pytest.mark.parametrize("name", NAMES)
def test_header_follows_the_naming_rule(name):
    from mantaflow_amd import _lib
    e = _lib.extension(name)
    assert (e.version_fn, e.version_macro) == ("mf_%s_abi_version" % name, "MF_%s_ABI_VERSION" % name.upper())
    assert re.search(r"^#define\s+%s\s+\d+\s*$" % e.version_macro, open(e.header).read(), flags=re.M)
    restype, argtypes, _ = _lib.parse_header(e.header)[e.version_fn]
    assert restype is ctypes.c_int and argtypes == []


def test_header_names_are_pairwise_disjoint():
    from mantaflow_amd import _lib
    seen = {n: "manta_hip.h" for n in _lib.parse_header()}
    for e in _lib.EXTENSIONS:
        protos = _lib.parse_header(e.header)
        assert protos
        for n in protos:
            assert n not in seen, "%s is declared by %s and by %s" % (n, seen[n], os.path.basename(e.header))
            seen[n] = os.path.basename(e.header)


def test_cpu_backend_has_no_extension_and_the_solver_mirrors_every_flag(oracle_backend):
    import manta as m
    from mantaflow_amd import _lib
    lib = _lib.get()
    s = m.Solver(name="o", gridSize=m.vec3(12, 10, 8), dim=3)
    for name in NAMES:
        assert getattr(lib, name) is False and getattr(s.lib, name) is False
    for flag, name in enumerate(NAMES):      # a mirror, not seven constants
        setattr(lib, name, flag % 2 == 0)
    try:
        mirrored = m.Solver(name="p", gridSize=m.vec3(12, 10, 8), dim=3).lib
        assert [getattr(mirrored, name) for name in NAMES] == [flag % 2 == 0 for flag in range(len(NAMES))]
    finally:
        for name in NAMES:
            setattr(lib, name, False)


def _calls(m, s, dims):
    """extension -> a call of its plugin on grids of solver s, and every object the calls could write"""
    flags, phi, real, lam = s.create(m.FlagGrid), s.create(m.LevelsetGrid), s.create(m.RealGrid), s.create(m.RealGrid)
    vel, vel2, vec, gpi = s.create(m.MACGrid), s.create(m.MACGrid), s.create(m.VecGrid), s.create(m.IntGrid)
    pp, pindex = s.create(m.BasicParticleSystem), s.create(m.ParticleIndexSystem)
    flags.initDomain(boundaryWidth=1)
    flags.fillGrid()
    phi.setConst(4.25)
    real.setConst(7.5)
    lam.setConst(2.0)
    vel.setConst(m.vec3(0.25, -0.5, 0.125))
    vel2.setConst(m.vec3(1, 2, 3))
    vec.setConst(m.vec3(3, 2, 1))
    pp.set_positions(np.random.RandomState(0).uniform(1, 7, (50, 3)) * (1, 1, 1 if dims[2] > 1 else 0))
    m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
    calls = {
        "obstacles": lambda: m.updateFractions(flags=flags, phiObs=phi, fractions=vel, boundaryWidth=1),
        "multigrid": lambda: m.solvePressure(vel=vel, pressure=real, flags=flags, preconditioner=m.PcMGStatic),
        "resample": lambda: m.combineGridVel(vel=vel, weight=vec, combineVel=vel2, phi=phi, narrowBand=2),
        "idp": lambda: m.computeDeltaX(deltaX=vel, Lambda=lam, flags=flags),
        "partls": lambda: m.averagedParticleLevelset(pp, pindex, flags, gpi, phi, 1.0, 1, 1),
        "guiding": lambda: m.PD_fluid_guiding(vel=vel, velT=vel2, pressure=real, flags=flags, weight=lam, blurRadius=2),
        "secparts": lambda: m.setMACFromLevelset(vel, phi, m.vec3(1, 2, 3)),
    }
    return calls, (flags, phi, real, lam, vel, vel2, vec, gpi)


def _refused(call, message, grids):
    before = [g.to_numpy().copy() for g in grids]
    live = grids[0].parent._live
    with pytest.raises(RuntimeError) as err:
        call()
    assert str(err.value) == message
    for g, b in zip(grids, before):
        assert (g.to_numpy() == b).all()
    assert grids[0].parent._live == live          # no scratch grid was taken


@pytest.fixture
def no_blur_precomp():
    import manta as m
    m.releaseBlurPrecomp()
    yield
    m.releaseBlurPrecomp()


@pytest.mark.parametrize("name", NAMES)
def test_one_plugin_of_each_extension_refuses_by_the_table(oracle_backend, no_blur_precomp, name):
    import manta as m
    dims = (12, 10, 8)
    s = m.Solver(name="o", gridSize=m.vec3(*dims), dim=3)
    calls, grids = _calls(m, s, dims)
    _refused(calls[name], _backend_message(name), grids)
    s._slab_window = (4, 40)      # what slab.SlabDomain gives the solver of a z-slab: (z offset, global sz)
    try:
        _refused(calls[name], _slab_message(name), grids)      # the z-slab check comes first
    finally:
        s._slab_window = (0, 0)


def test_multigrid_on_a_2d_solver_is_refused_for_the_backend_first(oracle_backend):
    import manta as m
    dims = (12, 10, 1)
    s = m.Solver(name="o", gridSize=m.vec3(*dims), dim=2)
    calls, grids = _calls(m, s, dims)
    _refused(calls["multigrid"], _backend_message("multigrid"), grids)


def test_compress_refuses_with_the_resampling_phrase(oracle_backend):
    import manta as m
    s = m.Solver(name="o", gridSize=m.vec3(12, 10, 8), dim=3)
    pp = s.create(m.BasicParticleSystem)
    pp.set_positions(np.full((4, 3), 3.5))
    with pytest.raises(RuntimeError) as err:
        pp.compress()
    assert str(err.value) == "compress: the 'oracle' backend does not implement particle resampling (manta_hip_resample.h)"
