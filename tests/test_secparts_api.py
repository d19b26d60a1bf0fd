"""Public surface of the secondary particles, without a GPU: names, signatures and defaults of the reference
(plugin/secondaryparticles.cpp:93-96, 202-206, 425-429, 471-472, 519-520, 530-531), the refusals on the CPU checker backend and on a
z-slab solver (before anything is touched), the ValueError of an unknown mode, radius < 1, the process-wide random streams of the two
sampling modes, and the C ABI extension include/manta_hip_secparts.h: it parses, shares no name with the other headers, and a library
binds all of it or none."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import secparts_model as M
import util

NAMES = ("flipComputeSecondaryParticlePotentials", "flipSampleSecondaryParticles", "flipUpdateSecondaryParticles",
         "flipDeleteParticlesInObstacle", "setFlagsFromLevelset", "setMACFromLevelset")
ENTRIES = {"mf_secparts_abi_version", "mf_secparts_potentials", "mf_secparts_scan_bytes", "mf_secparts_sample_plan", "mf_secparts_sample_emit",
           "mf_secparts_update", "mf_secparts_delete_in_obstacle", "mf_secparts_flags_from_levelset", "mf_secparts_mac_from_levelset"}


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_public_names_and_signatures():
    import manta as m
    E = inspect.Parameter.empty
    req = lambda *names: [(n, E) for n in names]
    assert _params(m.flipComputeSecondaryParticlePotentials) == req(
        "potTA", "potWC", "potKE", "neighborRatio", "flags", "v", "normal", "phi", "radius", "tauMinTA", "tauMaxTA", "tauMinWC", "tauMaxWC",
        "tauMinKE", "tauMaxKE", "scaleFromManta") + [("itype", m.FlagFluid), ("jtype", m.FlagObstacle | m.FlagOutflow | m.FlagInflow)]
    assert _params(m.flipSampleSecondaryParticles) == req(
        "mode", "flags", "v", "pts_sec", "v_sec", "l_sec", "lMin", "lMax", "potTA", "potWC", "potKE", "neighborRatio", "c_s", "c_b", "k_ta",
        "k_wc") + [("dt", 0), ("itype", m.FlagFluid)]
    assert _params(m.flipUpdateSecondaryParticles) == req(
        "mode", "pts_sec", "v_sec", "l_sec", "f_sec", "flags", "v", "neighborRatio", "radius", "gravity", "k_b", "k_d", "c_s", "c_b") + [
        ("dt", 0), ("scale", True), ("exclude", m.PtypeTracer), ("antitunneling", 0), ("itype", m.FlagFluid)]
    assert _params(m.flipDeleteParticlesInObstacle) == req("pts", "flags")
    assert _params(m.setFlagsFromLevelset) == req("flags", "phi") + [("exclude", m.FlagObstacle), ("itype", m.FlagFluid)]
    assert _params(m.setMACFromLevelset) == req("v", "phi", "c")
    ns = {}
    exec("from manta import *", ns)
    for n in NAMES + ("resetSecondaryParticleStreams",):
        assert n in ns, n
    # dt takes a fraction: its default must not make the plugin wrapper demand an int
    assert isinstance(inspect.signature(m.flipSampleSecondaryParticles).parameters["dt"].default, float)
    assert isinstance(inspect.signature(m.flipUpdateSecondaryParticles).parameters["dt"].default, float)


def test_header_declares_the_extension():
    from mantaflow_amd import _lib
    protos = _lib.parse_header(_lib.SECPARTS_HEADER)
    assert set(protos) == ENTRIES
    for name, (restype, argtypes, argnames) in protos.items():
        assert restype is ctypes.c_int
        if name not in ("mf_secparts_abi_version", "mf_secparts_scan_bytes"):
            assert argnames[-1] == "stream" and argtypes[-1] is ctypes.c_void_p, name
    assert len(protos["mf_secparts_potentials"][1]) == 26 and len(protos["mf_secparts_update"][1]) == 28
    for other in [_lib.HEADER] + [e.header for e in _lib.EXTENSIONS if e.name != "secparts"]:
        assert not set(protos) & set(_lib.parse_header(other))
    text = open(_lib.SECPARTS_HEADER).read()
    assert re.search(r"#define\s+MF_SECPARTS_ABI_VERSION\s+1\b", text)
    # the frozen header stays as it is
    assert "secparts" not in open(_lib.HEADER).read()


def test_product_library_exports_the_whole_extension():
    from mantaflow_amd import _lib
    assert os.path.exists(util.HIP_LIB), "%s missing -- run __graft_entry__.build()" % util.HIP_LIB
    L = ctypes.CDLL(util.HIP_LIB)          # loads without a GPU; no compute call is made here
    for name in ENTRIES:
        assert hasattr(L, name), name
    want = int(re.search(r"#define\s+MF_SECPARTS_ABI_VERSION\s+(\d+)", open(_lib.SECPARTS_HEADER).read()).group(1))
    assert L.mf_secparts_abi_version() == want


def test_extension_binds_as_a_whole_or_not_at_all(oracle_backend):
    from mantaflow_amd import _lib
    lib = _lib.get()
    assert lib.secparts is False          # the CPU checker has none of it, and still loads
    hip = ctypes.CDLL(util.HIP_LIB)

    class Part(object):
        """a library that exports one entry of the extension only"""
        mf_secparts_abi_version = hip.mf_secparts_abi_version

    saved = lib.cdll
    lib.cdll = Part()
    try:
        with pytest.raises(RuntimeError, match=r"implements part of manta_hip_secparts.h, lacks: "):
            lib._bind_extension("x.so", _lib.SECPARTS_HEADER, "mf_secparts_abi_version", "MF_SECPARTS_ABI_VERSION")
        lib.cdll = hip
        assert lib._bind_extension("x.so", _lib.SECPARTS_HEADER, "mf_secparts_abi_version", "MF_SECPARTS_ABI_VERSION") is True
    finally:
        lib.cdll = saved


class Objects(object):
    def __init__(self, m, dims):
        s = self.s = m.Solver(name="o", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)
        self.flags, self.vel, self.normal, self.phi = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.VecGrid), s.create(m.LevelsetGrid)
        self.pots = [s.create(m.RealGrid) for _ in range(4)]
        self.flags.initDomain(boundaryWidth=0)
        self.flags.fillGrid()
        for g in self.pots:
            g.setConst(0.75)
        self.phi.setConst(-0.5)
        self.vel.setConst(m.vec3(0.25, 0.5, 0.0))
        self.sec = s.create(m.BasicParticleSystem)
        self.sec.set_positions(np.random.RandomState(0).uniform(2, 6, (30, 3)) * (1, 1, 1 if dims[2] > 1 else 0))
        self.vSec, self.lSec, self.fSec = self.sec.create(m.PdataVec3), self.sec.create(m.PdataReal), self.sec.create(m.PdataVec3)
        self.lSec.setConst(2.0)

    def snapshot(self):
        return [g.to_numpy().copy() for g in [self.flags, self.vel, self.normal, self.phi] + self.pots] + [
            self.sec.get_positions(), self.sec.get_flags(), self.vSec.to_numpy(), self.lSec.to_numpy(), np.array([self.sec.pySize(), self.sec.mDeletes])]

    def calls(self, m):
        p = self.pots
        return {
            "flipComputeSecondaryParticlePotentials": lambda: m.flipComputeSecondaryParticlePotentials(
                p[0], p[1], p[2], p[3], self.flags, self.vel, self.normal, self.phi, 1, 0.1, 1.0, 0.1, 1.0, 0.1, 1.0, 0.1),
            "flipSampleSecondaryParticles": lambda: m.flipSampleSecondaryParticles(
                "single", self.flags, self.vel, self.sec, self.vSec, self.lSec, 1.0, 2.0, p[0], p[1], p[2], p[3], 0.3, 0.7, 10.0, 10.0, dt=0.5),
            "flipUpdateSecondaryParticles": lambda: m.flipUpdateSecondaryParticles(
                "linear", self.sec, self.vSec, self.lSec, self.fSec, self.flags, self.vel, p[3], 1, (0, -0.01, 0), 0.5, 0.5, 0.3, 0.7, dt=0.5),
            "flipDeleteParticlesInObstacle": lambda: m.flipDeleteParticlesInObstacle(self.sec, self.flags),
            "setFlagsFromLevelset": lambda: m.setFlagsFromLevelset(self.flags, self.phi),
            "setMACFromLevelset": lambda: m.setMACFromLevelset(self.vel, self.phi, (1, 2, 3)),
        }


def _refused(m, o, pattern):
    from mantaflow_amd import plugins
    plugins.resetSecondaryParticleStreams()
    before = o.snapshot()
    live = o.s._live
    for name, call in o.calls(m).items():
        with pytest.raises(RuntimeError, match=name + ": " + pattern):
            call()
    for a, b in zip(before, o.snapshot()):
        assert np.array_equal(a, b)
    assert o.s._live == live                                      # no scratch grid was taken
    assert plugins._secondary_stream("single").cursor == 0        # and no random number drawn


@pytest.mark.parametrize("dims", [(12, 10, 8), (15, 12, 1)])
def test_cpu_backend_refuses_the_plugins(oracle_backend, dims):
    import manta as m
    _refused(m, Objects(m, dims), r"the 'oracle' backend does not implement the secondary particles")


def test_z_slab_solver_refuses_the_plugins(oracle_backend):
    import manta as m
    o = Objects(m, (12, 10, 8))
    o.s._slab_window = (4, 40)      # what slab.SlabDomain gives the solver of a z-slab: (z offset, global sz)
    try:
        _refused(m, o, r"the secondary particles do not run on a z-slab solver")
    finally:
        o.s._slab_window = (0, 0)


class _FakeSecparts(object):
    """a stand-in for the solver's library that claims the extension: reaching a kernel entry is a test failure"""
    secparts, backend = True, "fake"

    def call(self, name, *a):
        raise AssertionError("reached %s" % name)


def test_unknown_mode_and_small_radius(oracle_backend):
    import manta as m
    o = Objects(m, (12, 10, 8))
    p = o.pots
    before = o.snapshot()
    with pytest.raises(ValueError, match=re.escape('Unknown mode: use "single" or "multiple" instead!')):
        m.flipSampleSecondaryParticles("double", o.flags, o.vel, o.sec, o.vSec, o.lSec, 1.0, 2.0, p[0], p[1], p[2], p[3], 0.3, 0.7, 10.0, 10.0)
    with pytest.raises(ValueError, match=re.escape('Unknown mode: use "linear" or "cubic" instead!')):
        m.flipUpdateSecondaryParticles("quadratic", o.sec, o.vSec, o.lSec, o.fSec, o.flags, o.vel, p[3], 1, (0, -0.01, 0), 0.5, 0.5, 0.3, 0.7)
    o.s.lib = _FakeSecparts()           # past the backend check: radius < 1 is refused before any entry is called
    for radius in (0, -1):
        with pytest.raises(RuntimeError, match=r"flipComputeSecondaryParticlePotentials: radius -?\d+ < 1"):
            m.flipComputeSecondaryParticlePotentials(p[0], p[1], p[2], p[3], o.flags, o.vel, o.normal, o.phi, radius, 0.1, 1.0, 0.1, 1.0, 0.1, 1.0, 0.1)
    for a, b in zip(before, o.snapshot()):
        assert np.array_equal(a, b)


def test_argument_types_are_checked(oracle_backend):
    import manta as m
    o = Objects(m, (12, 10, 8))
    p = o.pots
    with pytest.raises(RuntimeError, match="can't convert argument to MACGrid"):
        m.setMACFromLevelset(o.normal, o.phi, (1, 2, 3))
    with pytest.raises(RuntimeError, match="can't convert argument to FlagGrid"):
        m.flipDeleteParticlesInObstacle(o.sec, o.phi)
    with pytest.raises(RuntimeError, match=r"can't convert argument to ParticleDataImpl<Real>"):
        m.flipSampleSecondaryParticles("single", o.flags, o.vel, o.sec, o.vSec, o.vSec, 1.0, 2.0, p[0], p[1], p[2], p[3], 0.3, 0.7, 10.0, 10.0)
    with pytest.raises(RuntimeError, match="argument is not an int"):
        m.flipUpdateSecondaryParticles("linear", o.sec, o.vSec, o.lSec, o.fSec, o.flags, o.vel, p[3], 1, (0, -0.01, 0), 0.5, 0.5, 0.3, 0.7,
                                       antitunneling=1.5)
    with pytest.raises(RuntimeError, match="unknown"):
        m.setFlagsFromLevelset(o.flags, o.phi, jtype=1)


def test_streams_continue_across_calls_and_restart_on_reset():
    from mantaflow_amd import plugins
    plugins.resetSecondaryParticleStreams()
    want = M.Stream().take(40)
    s = plugins._secondary_stream("single")
    a, b = s.take(7), s.take(13)
    assert s.cursor == 20 and np.array_equal(np.concatenate([a, b]), want[:20])          # one stream, continued
    assert np.array_equal(plugins._secondary_stream("multiple").take(5), want[:5])        # one per mode
    assert np.array_equal(plugins._secondary_stream("single").take(20), want[20:40])
    plugins._set_secondary_stream_cursor("single", 11)
    assert plugins._secondary_stream("single").cursor == 11 and np.array_equal(plugins._secondary_stream("single").take(9), want[11:20])
    plugins.resetSecondaryParticleStreams()
    assert plugins._secondary_stream("single").cursor == 0 and plugins._secondary_stream("multiple").cursor == 0
    assert np.array_equal(plugins._secondary_stream("single").take(40), want)
    plugins.resetSecondaryParticleStreams()
