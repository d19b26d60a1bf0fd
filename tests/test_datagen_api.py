"""CPU: the public face of the smoke data-generation plugins without a GPU -- the six names and projectImage with their signatures,
the row of the open extension table with its header under include/open/, the kernels' file in the Makefile, both refusals of every
plugin (before anything is touched and before any scratch grid is taken) and the ValueErrors, raised before the library is called
(the validation is host code: it runs here with the library behind it replaced by one that fails on any call)."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest

WHAT = "the smoke data-generation plugins"
f32 = np.float32

SIGNATURES = {
    "blurMacGrid": "(oG, tG, si)",
    "blurRealGrid": "(oG, tG, si)",
    "calcCenterOfMass": "(density)",
    "projectPpmFull": "(val, name, shadeMode=0, scale=1.0)",
    "projectImage": "(val, shadeMode=0, scale=1.0)",
    "getLaplacian": "(laplacian, grid)",
    "getCurvature": "(curv, grid, h=1.0)",
}
ENTRIES = {"mf_datagen_abi_version", "mf_datagen_weights", "mf_datagen_blur", "mf_datagen_center_of_mass", "mf_datagen_project",
           "mf_datagen_laplacian", "mf_datagen_curvature"}


def test_names_and_signatures():
    import manta as m
    for name, sig in SIGNATURES.items():
        assert str(inspect.signature(getattr(m, name))) == sig, name
    # what other files pin as absent stays absent
    for name in ("obstacleLevelset", "obstacleGradient", "reinitMarching", "particleSurfaceTurbulence", "VortexSheetMesh", "VICintegration",
                 "smoothVorticity", "vorticitySource", "texcoordInflow", "meshSmokeInflow", "resampeOverfullCells", "dissolveSmoke",
                 "quantizeGrid", "resampleVec3ToMac"):
        assert not hasattr(m, name), name


def test_row_header_and_version_macro():
    from mantaflow_amd import _lib
    e = _lib.extension("datagen")
    assert e in _lib.OPEN_EXTENSIONS and (e.what, e.verb) == (WHAT, "do")
    inc = os.path.dirname(_lib.HEADER)
    assert e.header == os.path.join(inc, "open", "manta_hip_datagen.h") == _lib.DATAGEN_HEADER and os.path.exists(e.header)
    assert {x.header for x in _lib.OPEN_EXTENSIONS} == set(glob.glob(os.path.join(inc, "open", "manta_hip_*.h")))
    assert (e.version_fn, e.version_macro) == ("mf_datagen_abi_version", "MF_DATAGEN_ABI_VERSION")
    assert re.search(r"^#define\s+MF_DATAGEN_ABI_VERSION\s+1\s*$", open(e.header).read(), flags=re.M)
    restype, argtypes, _ = _lib.parse_header(e.header)[e.version_fn]
    assert restype is ctypes.c_int and argtypes == []


def test_entry_names_are_disjoint_from_every_other_header():
    from mantaflow_amd import _lib
    seen = {n: "manta_hip.h" for n in _lib.parse_header()}
    for e in _lib.all_extensions():
        if e.name != "datagen":
            for n in _lib.parse_header(e.header):
                seen[n] = os.path.basename(e.header)
    mine = _lib.parse_header(_lib.DATAGEN_HEADER)
    assert set(mine) == ENTRIES and all(n.startswith("mf_datagen_") for n in mine)
    for n in mine:
        assert n not in seen, "%s is declared by %s as well" % (n, seen.get(n))


def test_the_kernels_are_built_into_the_library():
    from mantaflow_amd import _lib
    csrc = os.path.join(os.path.dirname(_lib.DEFAULT_LIB))
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1).split()
    assert "datagen.hip" in srcs and os.path.exists(os.path.join(csrc, "datagen.hip"))
    text = open(os.path.join(csrc, "datagen.hip")).read()
    for n in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
    assert "hipcub" not in text and "rocprim" not in text
    assert "-ffp-contract=off" in open(os.path.join(csrc, "Makefile")).read()


def test_cpu_backend_lacks_the_extension(oracle_backend):
    import manta as m
    from mantaflow_amd import _lib
    assert _lib.get().datagen is False
    assert m.Solver(name="o", gridSize=m.vec3(8, 7, 6), dim=3).lib.datagen is False


# ---- a small scene on the CPU backend ---------------------------------------------------------------------------------------------
DIMS = (7, 5, 4)


class Stage(object):
    def __init__(self, m, tmp_path):
        sx, sy, sz = DIMS
        s = self.s = m.Solver(name="o", gridSize=m.vec3(*DIMS), dim=3)
        self.real, self.real2, self.phi = s.create(m.RealGrid), s.create(m.RealGrid), s.create(m.LevelsetGrid)
        self.mac, self.mac2, self.vec, self.flags = s.create(m.MACGrid), s.create(m.MACGrid), s.create(m.VecGrid), s.create(m.FlagGrid)
        self.grids = dict(real=self.real, real2=self.real2, phi=self.phi, mac=self.mac, mac2=self.mac2, vec=self.vec)
        rng = np.random.RandomState(5)
        for g in (self.real, self.real2, self.phi):
            g.from_numpy(rng.rand(sz, sy, sx).astype(f32))
        for g in (self.mac, self.mac2, self.vec):
            g.from_numpy(rng.rand(sz, sy, sx, 3).astype(f32))
        self.path = str(tmp_path / "out.ppm")

    def snapshot(self):
        snap = {k: g.to_numpy().copy() for k, g in self.grids.items()}
        snap["live"] = self.s._live
        snap["pooled"] = {k: len(v) for k, v in self.s._pool.items()}
        snap["file"] = os.path.exists(self.path)
        return snap

    def unchanged(self, snap):
        now = self.snapshot()
        for k in snap:
            assert np.array_equal(now[k], snap[k]) if isinstance(snap[k], np.ndarray) else now[k] == snap[k], k


def calls(m, S):
    """name -> calls with good arguments and with bad ones: the refusals come before every check"""
    return {
        "blurMacGrid": (lambda: m.blurMacGrid(S.mac, S.mac2, 1.128), lambda: m.blurMacGrid(S.mac, S.mac, 0.5), lambda: m.blurMacGrid(S.mac, S.real, -1.0)),
        "blurRealGrid": (lambda: m.blurRealGrid(oG=S.real, tG=S.real2, si=0.564), lambda: m.blurRealGrid(S.real, S.real, float("nan"))),
        "calcCenterOfMass": (lambda: m.calcCenterOfMass(S.real), lambda: m.calcCenterOfMass(density=S.mac)),
        "projectPpmFull": (lambda: m.projectPpmFull(S.real, S.path, 0, 1.0), lambda: m.projectPpmFull(S.real, S.path, shadeMode=1, scale=4.0),
                           lambda: m.projectPpmFull(S.mac, "/nonexistent/dir/x.ppm")),
        "projectImage": (lambda: m.projectImage(S.real), lambda: m.projectImage(S.phi, 1, scale=0.5), lambda: m.projectImage(S.vec)),
        "getLaplacian": (lambda: m.getLaplacian(S.real2, S.real), lambda: m.getLaplacian(S.real, S.real)),
        "getCurvature": (lambda: m.getCurvature(S.real2, S.phi, 0.5), lambda: m.getCurvature(curv=S.phi, grid=S.phi, h=1.0)),
    }


def test_the_stage_covers_every_plugin(oracle_backend, tmp_path):
    import manta as m
    assert set(calls(m, Stage(m, tmp_path))) == set(SIGNATURES)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_refused_on_the_cpu_backend_and_on_a_z_slab_solver(oracle_backend, tmp_path, name):
    import manta as m
    S = Stage(m, tmp_path)
    snap = S.snapshot()
    for call in calls(m, S)[name]:
        with pytest.raises(RuntimeError) as err:
            call()
        assert str(err.value) == "%s: the 'oracle' backend does not implement %s (manta_hip_datagen.h)" % (name, WHAT)
        S.unchanged(snap)
        S.s._slab_window = (4, 40)      # what slab.SlabDomain gives the solver of a z-slab: (z offset, global sz)
        try:
            with pytest.raises(RuntimeError) as err:
                call()
            assert str(err.value) == "%s: %s do not run on a z-slab solver" % (name, WHAT)      # the z-slab check comes first
        finally:
            S.s._slab_window = (0, 0)
        S.unchanged(snap)


# ---- validation: host code, run here with a library that fails on any call -------------------------------------------------------
class Untouchable(object):
    backend = "hip"

    def call(self, name, *args):
        raise AssertionError("%s was called: the validation let the arguments through" % name)


@pytest.fixture()
def validating(oracle_backend, monkeypatch, tmp_path):
    import manta as m
    from mantaflow_amd import plugins
    monkeypatch.setattr(plugins, "_extension_lib", lambda s, name, ext: Untouchable())
    return m, Stage(m, tmp_path)


def raises(S, exc, call, pattern):
    snap = S.snapshot()
    with pytest.raises(exc, match=pattern):
        call()
    S.unchanged(snap)


@pytest.mark.parametrize("si", [0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-50])
def test_sigma_must_be_positive(validating, si):
    m, S = validating
    raises(S, ValueError, lambda: m.blurRealGrid(S.real, S.real2, si), r"^blurRealGrid: sigma must be positive$")
    raises(S, ValueError, lambda: m.blurMacGrid(S.mac, S.mac, si), r"^blurMacGrid: sigma must be positive$")


def test_stencil_outputs_may_not_alias(validating):
    m, S = validating
    raises(S, ValueError, lambda: m.getLaplacian(S.real, S.real), r"^getLaplacian: the output grid must not be the input grid$")
    raises(S, ValueError, lambda: m.getCurvature(S.phi, S.phi), r"^getCurvature: the output grid must not be the input grid$")
    raises(S, ValueError, lambda: m.getCurvature(S.phi, S.phi, h=0.5), r"^getCurvature: the output grid must not be the input grid$")


def test_argument_types_and_sizes(validating):
    m, S = validating
    raises(S, RuntimeError, lambda: m.blurRealGrid(S.real, S.mac, 1.0), r"^can't convert argument to Grid<Real>\*$")
    raises(S, RuntimeError, lambda: m.blurRealGrid(S.flags, S.real, 1.0), r"^can't convert argument to Grid<Real>\*$")
    raises(S, RuntimeError, lambda: m.blurMacGrid(S.vec, S.mac, 1.0), r"^can't convert argument to MACGrid\*$")
    raises(S, RuntimeError, lambda: m.blurMacGrid(None, None, 1.0), r"^blurMacGrid: can't convert argument to a grid$")
    raises(S, RuntimeError, lambda: m.calcCenterOfMass(S.mac), r"^can't convert argument to Grid<Real>\*$")
    raises(S, RuntimeError, lambda: m.projectImage(S.vec), r"^can't convert argument to Grid<Real>\*$")
    raises(S, RuntimeError, lambda: m.projectImage(S.real, shadeMode=0.5), r"^argument is not an int$")
    raises(S, RuntimeError, lambda: m.getLaplacian(S.mac, S.real), r"^can't convert argument to Grid<Real>\*$")
    raises(S, RuntimeError, lambda: m.getCurvature(S.real, S.flags), r"^can't convert argument to Grid<Real>\*$")
    other = m.Solver(name="p", gridSize=m.vec3(8, 5, 4), dim=3)
    raises(S, RuntimeError, lambda: m.blurRealGrid(S.real, other.create(m.RealGrid), 1.0), r"^different grid resolutions")
    raises(S, RuntimeError, lambda: m.getCurvature(other.create(m.RealGrid), S.phi), r"^different grid resolutions")


def test_good_arguments_reach_the_library(validating):
    """the other side of the validation tests: with good arguments every plugin gets as far as its first library call, and the blurs
    hand their scratch back to the pool on the way out"""
    m, S = validating
    live = S.s._live
    for name, variants in calls(m, S).items():
        with pytest.raises(AssertionError, match="was called"):
            variants[0]()
        assert S.s._live == live, name
