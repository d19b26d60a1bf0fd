"""CPU: the public face of the array bridge and the MLFLIP data plugins without a GPU -- the 24 names and their signatures, the row of
the open extension table with its header under include/open/, the kernels' file in the Makefile, both refusals of every plugin (before
anything is touched, argument checks included), and every validation error of the array argument and of the plugins, raised before
the library is called and with the targets unchanged (the validation is host code: it runs here with the library behind it replaced by
one that fails on any call)."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mlflip_model as M

WHAT = "the array bridge and the MLFLIP plugins"
f32, f64, i32 = np.float32, np.float64, np.int32

FEATURE_SIG = "(fv, N_row, off_begin, p, %s, scale=1.0, ptype=None, exclude=0, window=1)"
SIGNATURES = {
    "extractFeatureVel": FEATURE_SIG % "vel",
    "extractFeaturePhi": FEATURE_SIG % "phi",
    "extractFeatureGeo": FEATURE_SIG % "flag",
    "getRegions": "(r, flags, ctype)",
    "getRegionalCounts": "(r, flags, ctype)",
    "extendRegion": "(flags, region, exclude, depth)",
    "markSmallRegions": "(flags, rcnt, mark, exclude, th=1)",
    "simpleNumpyTest": "(grid, npAr, scale)",
}
for _k in ("Real", "Flag", "Levelset", "Vec3", "MAC"):
    SIGNATURES["copyArrayToGrid" + _k] = SIGNATURES["copyGridToArray" + _k] = "(source, target)"
for _k in ("Int", "Real", "Vec3"):
    SIGNATURES["copyArrayToPdata" + _k] = SIGNATURES["copyPdataToArray" + _k] = "(source, target)"
ENTRIES = {"mf_mlflip_abi_version", "mf_mlflip_convert", "mf_mlflip_planes_to_elements", "mf_mlflip_elements_to_planes",
           "mf_mlflip_extract_feature", "mf_mlflip_regions", "mf_mlflip_extend_region", "mf_mlflip_mark_small_regions",
           "mf_mlflip_simple_array_add"}


def test_names_and_signatures():
    import manta as m
    assert len(SIGNATURES) == 24
    for name, sig in SIGNATURES.items():
        assert str(inspect.signature(getattr(m, name))) == sig, name
    # what other files pin as absent stays absent
    for name in ("obstacleLevelset", "obstacleGradient", "reinitMarching", "particleSurfaceTurbulence", "VortexSheetMesh", "VICintegration",
                 "smoothVorticity", "vorticitySource", "texcoordInflow", "meshSmokeInflow"):
        assert not hasattr(m, name), name
    assert callable(m.LevelsetGrid.reinitMarching)


def test_row_header_and_version_macro():
    from mantaflow_amd import _lib
    e = _lib.extension("mlflip")
    assert e in _lib.OPEN_EXTENSIONS and (e.what, e.verb) == (WHAT, "do")
    inc = os.path.dirname(_lib.HEADER)
    assert e.header == os.path.join(inc, "open", "manta_hip_mlflip.h") == _lib.MLFLIP_HEADER and os.path.exists(e.header)
    assert {x.header for x in _lib.OPEN_EXTENSIONS} == set(glob.glob(os.path.join(inc, "open", "manta_hip_*.h")))
    assert (e.version_fn, e.version_macro) == ("mf_mlflip_abi_version", "MF_MLFLIP_ABI_VERSION")
    assert re.search(r"^#define\s+MF_MLFLIP_ABI_VERSION\s+\d+\s*$", open(e.header).read(), flags=re.M)
    restype, argtypes, _ = _lib.parse_header(e.header)[e.version_fn]
    assert restype is ctypes.c_int and argtypes == []


def test_entry_names_are_disjoint_from_every_other_header():
    from mantaflow_amd import _lib
    seen = {n: "manta_hip.h" for n in _lib.parse_header()}
    for e in _lib.all_extensions():
        if e.name != "mlflip":
            for n in _lib.parse_header(e.header):
                seen[n] = os.path.basename(e.header)
    mine = _lib.parse_header(_lib.MLFLIP_HEADER)
    assert set(mine) == ENTRIES and all(n.startswith("mf_mlflip_") for n in mine)
    for n in mine:
        assert n not in seen, "%s is declared by %s as well" % (n, seen.get(n))


def test_the_kernels_are_built_into_the_library():
    from mantaflow_amd import _lib
    csrc = os.path.join(os.path.dirname(_lib.DEFAULT_LIB))
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1).split()
    assert "mlflip.hip" in srcs and os.path.exists(os.path.join(csrc, "mlflip.hip"))
    text = open(os.path.join(csrc, "mlflip.hip")).read()
    for n in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
    assert "hipcub" not in text and "rocprim" not in text            # the scan comes through scan.h


def test_cpu_backend_lacks_the_extension(oracle_backend):
    import manta as m
    from mantaflow_amd import _lib
    assert _lib.get().mlflip is False
    assert m.Solver(name="o", gridSize=m.vec3(8, 7, 6), dim=3).lib.mlflip is False


# ---- a small scene on the CPU backend: every plugin with good arguments, and with bad ones ---------------------------------------
DIMS = (7, 5, 4)
NP = 5


class Stage(object):
    def __init__(self, m):
        sx, sy, sz = DIMS
        n = sx * sy * sz
        s = self.s = m.Solver(name="o", gridSize=m.vec3(*DIMS), dim=3)
        self.real, self.flags, self.phi = s.create(m.RealGrid), s.create(m.FlagGrid), s.create(m.LevelsetGrid)
        self.vec, self.mac, self.r = s.create(m.VecGrid), s.create(m.MACGrid), s.create(m.IntGrid)
        self.grids = dict(real=self.real, flags=self.flags, phi=self.phi, vec=self.vec, mac=self.mac, r=self.r)
        rng = np.random.RandomState(3)
        self.real.from_numpy(rng.rand(sz, sy, sx).astype(f32))
        self.phi.from_numpy(rng.rand(sz, sy, sx).astype(f32))
        self.flags.from_numpy(M.random_flags(DIMS, 0.5, 1))
        self.r.from_numpy(rng.randint(0, 9, (sz, sy, sx)).astype(i32))
        self.vec.from_numpy(rng.rand(sz, sy, sx, 3).astype(f32))
        self.mac.from_numpy(rng.rand(sz, sy, sx, 3).astype(f32))
        self.pp = s.create(m.BasicParticleSystem)
        self.pI, self.pR, self.pV = self.pp.create(m.PdataInt), self.pp.create(m.PdataReal), self.pp.create(m.PdataVec3)
        self.pp.set_positions(f32(1.5) + rng.rand(NP, 3).astype(f32) * f32(1.5))
        self.pI.from_numpy(np.arange(NP, dtype=i32))
        self.pR.from_numpy(rng.rand(NP).astype(f32))
        self.pV.from_numpy(rng.rand(NP, 3).astype(f32))
        self.pdata = dict(pI=self.pI, pR=self.pR, pV=self.pV)
        self.arrays = dict(
            a3=np.full((sz, sy, sx), 2.5, f32), a3i=np.full((sz, sy, sx), 3, i32), a3d=np.full((sz, sy, sx), 1.5, f64),
            a4=np.full((sz, sy, sx, 3), 0.5, f32), nI=np.full(NP, 7, i32), nR=np.full(NP, 0.25, f32), nV=np.full(3 * NP, 0.75, f32),
            fv=np.full(NP * 140, -1, f32), plane=np.full(sx * sy, 2, f32))

    def snapshot(self):
        snap = {k: g.to_numpy().copy() for k, g in self.grids.items()}
        snap.update({k: p.to_numpy().copy() for k, p in self.pdata.items()})
        snap.update({"arr/" + k: a.copy() for k, a in self.arrays.items()})
        snap["pos"] = self.pp.get_positions().copy()
        snap["live"] = self.s._live
        return snap

    def unchanged(self, snap):
        now = self.snapshot()
        for k in snap:
            assert np.array_equal(now[k], snap[k]), k


def calls(m, S):
    """name -> (a call with good arguments, a call with bad ones)"""
    A = S.arrays
    out = {}
    for kind, g, a in (("Real", S.real, "a3"), ("Flag", S.flags, "a3i"), ("Levelset", S.phi, "a3d"), ("Vec3", S.vec, "a4"), ("MAC", S.mac, "a4")):
        out["copyArrayToGrid" + kind] = (lambda g=g, a=a, k=kind: getattr(m, "copyArrayToGrid" + k)(source=A[a], target=g),
                                         lambda g=g, k=kind: getattr(m, "copyArrayToGrid" + k)(source=A["nR"], target=g))
        out["copyGridToArray" + kind] = (lambda g=g, a=a, k=kind: getattr(m, "copyGridToArray" + k)(source=g, target=A[a]),
                                         lambda g=g, k=kind: getattr(m, "copyGridToArray" + k)(source=g, target="no array"))
    for kind, p, a in (("Int", S.pI, "nI"), ("Real", S.pR, "nR"), ("Vec3", S.pV, "nV")):
        out["copyArrayToPdata" + kind] = (lambda p=p, a=a, k=kind: getattr(m, "copyArrayToPdata" + k)(source=A[a], target=p),
                                          lambda p=p, k=kind: getattr(m, "copyArrayToPdata" + k)(source=A["a3d"], target=p))
        out["copyPdataToArray" + kind] = (lambda p=p, a=a, k=kind: getattr(m, "copyPdataToArray" + k)(source=p, target=A[a]),
                                          lambda p=p, k=kind: getattr(m, "copyPdataToArray" + k)(source=p, target=A["plane"]))
    for name, grid in (("extractFeatureVel", S.mac), ("extractFeaturePhi", S.phi), ("extractFeatureGeo", S.flags)):
        out[name] = (lambda n=name, g=grid: getattr(m, n)(A["fv"], 140, 2, S.pp, g, 1.0, S.pI, 1, 1),
                     lambda n=name, g=grid: getattr(m, n)(A["fv"], 3, -1, S.pp, g, window=-2))
    out["getRegions"] = (lambda: m.getRegions(r=S.r, flags=S.flags, ctype=1), lambda: m.getRegions(r=S.real, flags=S.flags, ctype=1))
    out["getRegionalCounts"] = (lambda: m.getRegionalCounts(r=S.r, flags=S.flags, ctype=1), lambda: m.getRegionalCounts(r=S.r, flags=S.r, ctype=1))
    out["extendRegion"] = (lambda: m.extendRegion(flags=S.flags, region=4, exclude=2, depth=2), lambda: m.extendRegion(S.flags, 4, 2, 0.5))
    out["markSmallRegions"] = (lambda: m.markSmallRegions(flags=S.flags, rcnt=S.r, mark=4, exclude=2, th=3),
                               lambda: m.markSmallRegions(S.flags, S.real, 4, 2))
    out["simpleNumpyTest"] = (lambda: m.simpleNumpyTest(S.real, A["plane"], 0.5), lambda: m.simpleNumpyTest(S.real, A["nR"], 0.5))
    return out


def test_the_stage_covers_every_plugin(oracle_backend):
    import manta as m
    assert set(calls(m, Stage(m))) == set(SIGNATURES)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_refused_on_the_cpu_backend_and_on_a_z_slab_solver(oracle_backend, name):
    import manta as m
    S = Stage(m)
    snap = S.snapshot()
    for call in calls(m, S)[name]:
        with pytest.raises(RuntimeError) as err:
            call()
        assert str(err.value) == "%s: the 'oracle' backend does not implement %s (manta_hip_mlflip.h)" % (name, WHAT)
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
def validating(oracle_backend, monkeypatch):
    import manta as m
    from mantaflow_amd import plugins
    monkeypatch.setattr(plugins, "_extension_lib", lambda s, name, ext: Untouchable())
    return m, Stage(m)


def raises(S, call, pattern):
    snap = S.snapshot()
    with pytest.raises(RuntimeError, match=pattern):
        call()
    S.unchanged(snap)


def test_array_argument(validating):
    m, S = validating
    sx, sy, sz = DIMS
    good = S.arrays["a3"]
    raises(S, lambda: m.copyArrayToGridReal([[1.0]], S.real), r"^copyArrayToGridReal: can't convert argument to a numpy array or a torch tensor$")
    raises(S, lambda: m.copyGridToArrayReal(S.real, None), r"^copyGridToArrayReal: can't convert argument")
    for bad in (np.zeros((sz, sy, sx), np.int64), np.zeros((sz, sy, sx), np.float16), torch.zeros((sz, sy, sx), dtype=torch.int64),
                np.zeros((sz, sy, sx), ">f4"), np.zeros((sz, sy, sx), bool)):
        raises(S, lambda: m.copyArrayToGridReal(bad, S.real), r"^copyArrayToGridReal: unknown type of Numpy array$")
        raises(S, lambda: m.copyGridToArrayFlag(S.flags, bad), r"^copyGridToArrayFlag: unknown type of Numpy array$")
    # targets: C-contiguous and writable; sources may be anything
    fortran = np.asfortranarray(good)
    assert not fortran.flags["C_CONTIGUOUS"]
    raises(S, lambda: m.copyGridToArrayReal(S.real, fortran), r"^copyGridToArrayReal: target array must be C-contiguous$")
    raises(S, lambda: m.copyGridToArrayReal(S.real, torch.from_numpy(fortran)), r"^copyGridToArrayReal: target array must be C-contiguous$")
    raises(S, lambda: m.copyGridToArrayVec3(S.vec, np.zeros((sz, sy, sx, 6), f32)[..., ::2]), r"^copyGridToArrayVec3: target array must be C-contiguous$")
    raises(S, lambda: m.copyPdataToArrayReal(S.pR, np.zeros(2 * NP, f32)[::2]), r"^copyPdataToArrayReal: target array must be C-contiguous$")
    frozen = good.copy()
    frozen.setflags(write=False)
    raises(S, lambda: m.copyGridToArrayReal(S.real, frozen), r"^copyGridToArrayReal: target array is read-only$")
    # a tensor on a device that is not the solver's
    elsewhere = torch.empty((sz, sy, sx), dtype=torch.float32, device="meta")
    raises(S, lambda: m.copyArrayToGridReal(elsewhere, S.real), r"^copyArrayToGridReal: the tensor lives on meta, the solver on cpu$")
    raises(S, lambda: m.copyGridToArrayReal(S.real, elsewhere), r"^copyGridToArrayReal: the tensor lives on meta")
    # wrong objects
    raises(S, lambda: m.copyArrayToGridReal(good, S.flags), r"^can't convert argument to Grid<Real>\*$")
    raises(S, lambda: m.copyArrayToGridLevelset(good, S.real), r"^can't convert argument to LevelsetGrid\*$")
    raises(S, lambda: m.copyArrayToGridMAC(S.arrays["a4"], S.vec), r"^can't convert argument to MACGrid\*$")
    raises(S, lambda: m.copyArrayToGridReal(good, None), r"^copyArrayToGridReal: can't convert argument to a grid or particle object$")
    raises(S, lambda: m.copyArrayToPdataInt(S.arrays["nI"], S.pR), r"ParticleDataImpl<int>")


def test_grid_copy_sizes_shapes_and_types(validating):
    m, S = validating
    sx, sy, sz = DIMS
    n = sx * sy * sz
    small, flat, swapped = np.zeros((sz, sy, sx - 1), f32), np.zeros(n, f32), np.zeros((sx, sy, sz), f32)
    raises(S, lambda: m.copyArrayToGridReal(small, S.real), r"^copyArrayToGridReal: The size of the numpy array doesn't match the size of the Grid!$")
    raises(S, lambda: m.copyArrayToGridFlag(small, S.flags), r"^copyArrayToGridFlag: The size of the numpy array doesn't match the size of the Grid!$")
    raises(S, lambda: m.copyGridToArrayLevelset(S.phi, small),
           r"^copyGridToArrayLevelset: The size of the numpy array %d doesn't match the size of the grid!$" % small.size)
    raises(S, lambda: m.copyArrayToGridVec3(np.zeros((sz, sy, sx), f32), S.vec), r"^copyArrayToGridVec3: The size of the numpy array doesn't match the size of the grid!$")
    raises(S, lambda: m.copyGridToArrayMAC(S.mac, np.zeros((sz, sy, sx, 2), f32)), r"^copyGridToArrayMAC: The size of the numpy array doesn't match the size of the grid!$")
    raises(S, lambda: m.copyArrayToGridReal(swapped, S.real),
           r"^copyArrayToGridReal: The dimensions of source numpy array \(4, 5, 7\) and target grid \(7, 5, 4\) do not match!$")
    raises(S, lambda: m.copyGridToArrayReal(S.real, swapped),
           r"^copyGridToArrayReal: The dimensions of source grid \(7, 5, 4\) and target numpy array \(4, 5, 7\) do not match!$")
    raises(S, lambda: m.copyArrayToGridReal(flat, S.real), r"^copyArrayToGridReal: The dimensions of source numpy array \(0, 0, %d\)" % n)
    raises(S, lambda: m.copyArrayToGridVec3(np.zeros((sz, sy, 3 * sx), f32), S.vec), r"^copyArrayToGridVec3: The dimensions of source numpy array")
    raises(S, lambda: m.copyGridToArrayVec3(S.vec, np.zeros((sz * sy * sx, 3), f32)), r"^copyGridToArrayVec3: The dimensions of source grid")
    for plug, g in ((m.copyArrayToGridVec3, S.vec), (m.copyArrayToGridMAC, S.mac)):
        raises(S, lambda: plug(np.zeros((sz, sy, sx, 3), i32), g), r"^copyArrayToGrid(Vec3|MAC): unknown/unsupported type of Vec3 Numpy array$")
    raises(S, lambda: m.copyGridToArrayVec3(S.vec, np.zeros((sz, sy, sx, 3), i32)), r"^copyGridToArrayVec3: unknown/unsupported type of Vec3 Numpy array$")


def test_pdata_copy_sizes_and_types(validating):
    m, S = validating
    size = r": The size of the numpy array doesn't match the size of the pdata field!$"
    raises(S, lambda: m.copyArrayToPdataInt(np.zeros(NP + 1, i32), S.pI), "^copyArrayToPdataInt" + size)
    raises(S, lambda: m.copyPdataToArrayReal(S.pR, np.zeros(NP - 1, f32)), "^copyPdataToArrayReal" + size)
    raises(S, lambda: m.copyArrayToPdataVec3(np.zeros(NP, f32), S.pV), "^copyArrayToPdataVec3" + size)
    raises(S, lambda: m.copyPdataToArrayVec3(S.pV, np.zeros((NP, 2), f32)), "^copyPdataToArrayVec3" + size)
    raises(S, lambda: m.copyArrayToPdataInt(np.zeros(NP, f32), S.pI), r"^copyArrayToPdataInt: array of type float32 where int32 is needed$")
    raises(S, lambda: m.copyPdataToArrayInt(S.pI, np.zeros(NP, f64)), r"^copyPdataToArrayInt: array of type float64 where int32 is needed$")
    raises(S, lambda: m.copyArrayToPdataReal(np.zeros(NP, f64), S.pR), r"^copyArrayToPdataReal: array of type float64 where float32 is needed$")
    raises(S, lambda: m.copyPdataToArrayReal(S.pR, torch.zeros(NP, dtype=torch.int32)), r"^copyPdataToArrayReal: array of type int32 where float32 is needed$")
    raises(S, lambda: m.copyArrayToPdataVec3(np.zeros((NP, 3), f64), S.pV), r"^copyArrayToPdataVec3: array of type float64 where float32 is needed$")
    raises(S, lambda: m.copyPdataToArrayVec3(S.pV, np.zeros((NP, 3), i32)), r"^copyPdataToArrayVec3: array of type int32 where float32 is needed$")
    raises(S, lambda: m.copyPdataToArrayVec3(S.pV, np.zeros((NP, 3), np.int64)), r"^copyPdataToArrayVec3: array of type int64 where float32 is needed$")


@pytest.mark.parametrize("name,D", [("extractFeatureVel", 3), ("extractFeaturePhi", 1), ("extractFeatureGeo", 1)])
def test_feature_checks(validating, name, D):
    m, S = validating
    plug = getattr(m, name)
    grid = {"extractFeatureVel": S.mac, "extractFeaturePhi": S.phi, "extractFeatureGeo": S.flags}[name]
    need = 27 * D
    fv = np.full(NP * (need + 2), -1, f32)
    raises(S, lambda: plug(fv[:-1], need + 2, 0, S.pp, grid), r"^%s: the feature array holds %d values, %d rows of %d need %d$" % (name, fv.size - 1, NP, need + 2, fv.size))
    raises(S, lambda: plug(fv, need + 2, -1, S.pp, grid), r"^%s: 27 stencil points of %d values from column -1 do not fit a row of %d$" % (name, D, need + 2))
    raises(S, lambda: plug(fv, need + 2, 3, S.pp, grid), r"^%s: 27 stencil points of %d values from column 3 do not fit a row of %d$" % (name, D, need + 2))
    raises(S, lambda: plug(fv, need - 1, 0, S.pp, grid), r"^%s: 27 stencil points" % name)
    raises(S, lambda: plug(fv, need + 2, 0, S.pp, grid, window=-1), r"^%s: window -1$" % name)
    raises(S, lambda: plug(fv.astype(f64), need + 2, 0, S.pp, grid), r"^%s: array of type float64 where float32 is needed$" % name)
    raises(S, lambda: plug(np.zeros((NP, 2 * (need + 2)), f32)[:, ::2], need + 2, 0, S.pp, grid), r"^%s: target array must be C-contiguous$" % name)
    raises(S, lambda: plug(fv, need + 2, 0, S.pp, S.r), r"^can't convert argument to ")
    raises(S, lambda: plug(fv, need + 2, 0, S.pI, grid), r"^can't convert argument to BasicParticleSystem\*$")
    raises(S, lambda: plug(fv, need + 2, 0, S.pp, grid, ptype=S.pR), r"ParticleDataImpl<int>")
    # the window decides what fits: window 0 needs D values only
    raises(S, lambda: plug(fv, D, 1, S.pp, grid, window=0), r"^%s: 1 stencil points of %d values from column 1 do not fit a row of %d$" % (name, D, D))


def test_region_and_flag_plugin_checks(validating):
    m, S = validating
    raises(S, lambda: m.getRegions(S.real, S.flags, 1), r"^can't convert argument to Grid<int>\*$")
    raises(S, lambda: m.getRegions(S.r, S.r, 1), r"^can't convert argument to FlagGrid\*$")
    raises(S, lambda: m.getRegionalCounts(S.flags, S.flags, 1), r"^getRegionalCounts: r and flags are the same grid$")
    raises(S, lambda: m.extendRegion(S.r, 4, 2, 1), r"^can't convert argument to FlagGrid\*$")
    raises(S, lambda: m.extendRegion(S.flags, 4, 2, 1.5), r"^argument is not an int$")
    raises(S, lambda: m.markSmallRegions(S.flags, S.real, 4, 2), r"^can't convert argument to Grid<int>\*$")
    other = m.Solver(name="p", gridSize=m.vec3(8, 5, 4), dim=3)
    raises(S, lambda: m.getRegions(other.create(m.IntGrid), S.flags, 1), r"^different grid resolutions")
    raises(S, lambda: m.markSmallRegions(S.flags, other.create(m.IntGrid), 4, 2), r"^different grid resolutions")
    snap = S.snapshot()
    m.extendRegion(S.flags, 4, 2, 0)                 # no round: nothing to call
    m.extendRegion(S.flags, 4, 2, -3)
    S.unchanged(snap)


def test_simple_numpy_test_checks(validating):
    m, S = validating
    sx, sy, sz = DIMS
    raises(S, lambda: m.simpleNumpyTest(S.real, np.zeros(sx * sy - 1, f32), 1.0), r"^simpleNumpyTest: the array holds %d values, a plane of the grid has %d$" % (sx * sy - 1, sx * sy))
    raises(S, lambda: m.simpleNumpyTest(S.real, np.zeros(sx * sy, f64), 1.0), r"^simpleNumpyTest: array of type float64 where float32 is needed$")
    raises(S, lambda: m.simpleNumpyTest(S.flags, np.zeros(sx * sy, f32), 1.0), r"^can't convert argument to Grid<Real>\*$")


def test_good_arguments_reach_the_library(validating):
    """the other side of the validation tests: with good arguments every plugin gets as far as its first library call"""
    m, S = validating
    for name, (good, _) in calls(m, S).items():
        with pytest.raises(AssertionError, match="was called"):
            good()
