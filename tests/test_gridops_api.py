"""CPU: the public face of the grid operations without a GPU -- every new name with its signature, the row of the open extension table
with its header under include/open/, the kernels' file in the Makefile, both refusals of every kernel-backed name (before anything is
touched and before any scratch grid is taken), the permutation's refusals, and the host-only names against the fixture on the CPU
checker backend."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest

import gridops_model as M

WHAT = "the grid-operation plugins"
f32 = np.float32
GOLDEN = np.load(M.GOLDEN)

PLUGINS = {
    "addForceField": "(flags, vel, force, region=None, isMAC=False)",
    "setForceField": "(flags, vel, force, region=None, isMAC=False)",
    "setInitialVelocity": "(flags, vel, invel)",
    "extrapolateVec3Simple": "(vel, phi, distance=4, inside=False)",
    "applyEmission": "(flags, target, source, emissionTexture=None, isAbsolute=True, type=0)",
    "resetInObstacle": "(flags, vel, density, heat=None, fuel=None, flame=None, red=None, green=None, blue=None, resetValue=0)",
    "copyMACData": "(source, target, flags, flag, bnd)",
    "copyRealToVec3": "(sourceX, sourceY, sourceZ, target)",
    "copyVec3ToReal": "(source, targetX, targetY, targetZ)",
    "resampleMacToVec3": "(source, target)",
    "swapComponents": "(vel, c1=0, c2=1, c3=2)",
    "getGridAvg": "(source, flags=None)",
    "debugIntToReal": "(source, dest, factor=1.0)",
    "applySimpleNoiseReal": "(flags, target, noise, scale=1.0, weight=None)",
    "applySimpleNoiseVec3": "(flags, target, noise, scale=1.0, weight=None)",
    "printUniFileInfoString": "(name)",
    "getNpzFileSize": "(name)",
    "flipComputePotentialTrappedAir": "(pot, flags, v, radius, tauMin, tauMax, scaleFromManta, itype=1, jtype=1)",
    "flipComputePotentialKineticEnergy": "(pot, flags, v, tauMin, tauMax, scaleFromManta, itype=1)",
    "flipComputePotentialWaveCrest": "(pot, flags, v, radius, normal, tauMin, tauMax, scaleFromManta, itype=1, jtype=1)",
    "flipComputeSurfaceNormals": "(normal, phi)",
    "flipUpdateNeighborRatio": "(flags, neighborRatio, radius, itype=1, jtype=2)",
}
GRID_CLASSES = ("RealGrid", "IntGrid", "VecGrid", "MACGrid", "FlagGrid")
GRID_METHODS = {
    "permuteAxes": "(self, axis0, axis1, axis2)",
    "permuteAxesCopyToGrid": "(self, axis0, axis1, axis2, out)",
    "getL1": "(self, bnd=0)",
    "getL2": "(self, bnd=0)",
    "join": "(self, a, keepMax=True)",
    "get": "(self, i, j, k)",
    "set": "(self, i, j, k, val)",
    "get_name": "(self)",
    "set_name": "(self, s)",
    "getSizeT": "(self)",
    "getStrideT": "(self)",
}
OTHER_METHODS = {
    ("RealGrid", "getInterpolated"): "(self, pos)",
    ("LevelsetGrid", "getInterpolated"): "(self, pos)",
    ("VecGrid", "getInterpolated"): "(self, pos)",
    ("MACGrid", "getInterpolated"): "(self, pos)",
    ("MACGrid", "getCentered"): "(self, pos)",
    ("MACGrid", "getAtMACX"): "(self, i, j, k)",
    ("MACGrid", "getAtMACY"): "(self, i, j, k)",
    ("MACGrid", "getAtMACZ"): "(self, i, j, k)",
    ("BasicParticleSystem", "transformPositions"): "(self, dimOld, dimNew)",
    ("LevelsetGrid", "join"): "(self, o)",                      # LevelsetGrid.join keeps its own meaning
}
ENTRIES = {"mf_gridops_abi_version", "mf_gridops_permute", "mf_gridops_norm", "mf_gridops_join", "mf_gridops_force_field",
           "mf_gridops_add_force_if_lower", "mf_gridops_extrapolate_vec3_simple", "mf_gridops_apply_emission", "mf_gridops_reset_in_obstacle",
           "mf_gridops_copy_mac_data", "mf_gridops_copy_planes", "mf_gridops_resample_mac_to_vec3", "mf_gridops_swap_components",
           "mf_gridops_grid_avg", "mf_gridops_simple_noise", "mf_gridops_legacy_potential", "mf_gridops_neighbor_ratio",
           "mf_gridops_surface_normals", "mf_gridops_int_to_real"}


def test_names_and_signatures():
    import manta as m
    for name, sig in PLUGINS.items():
        assert str(inspect.signature(getattr(m, name))) == sig, name
    for cls in GRID_CLASSES:
        for name, sig in GRID_METHODS.items():
            assert str(inspect.signature(getattr(getattr(m, cls), name))) == sig, (cls, name)
    for (cls, name), sig in OTHER_METHODS.items():
        assert str(inspect.signature(getattr(getattr(m, cls), name))) == sig, (cls, name)
    assert m.WaveletNoiseField is m.NoiseField


def test_row_header_and_version_macro():
    from mantaflow_amd import _lib
    e = _lib.extension("gridops")
    assert e in _lib.OPEN_EXTENSIONS and (e.what, e.verb) == (WHAT, "do")
    inc = os.path.dirname(_lib.HEADER)
    assert e.header == os.path.join(inc, "open", "manta_hip_gridops.h") == _lib.GRIDOPS_HEADER and os.path.exists(e.header)
    assert {x.header for x in _lib.OPEN_EXTENSIONS} == set(glob.glob(os.path.join(inc, "open", "manta_hip_*.h")))
    assert (e.version_fn, e.version_macro) == ("mf_gridops_abi_version", "MF_GRIDOPS_ABI_VERSION")
    text = open(e.header).read()
    assert re.search(r"^#define\s+MF_GRIDOPS_ABI_VERSION\s+1\s*$", text, flags=re.M)
    # the tile of the transposing permutations: 32 x 32 words with a pitch of 33, the figures of the bank derivation
    assert re.search(r"^#define\s+MF_GRIDOPS_TILE\s+32\s*$", text, flags=re.M) and re.search(r"^#define\s+MF_GRIDOPS_TILE_PITCH\s+33\s*$", text, flags=re.M)
    restype, argtypes, _ = _lib.parse_header(e.header)[e.version_fn]
    assert restype is ctypes.c_int and argtypes == []


def test_entry_names_are_disjoint_from_every_other_header():
    from mantaflow_amd import _lib
    seen = {n: "manta_hip.h" for n in _lib.parse_header()}
    for e in _lib.all_extensions():
        if e.name != "gridops":
            for n in _lib.parse_header(e.header):
                seen[n] = os.path.basename(e.header)
    mine = _lib.parse_header(_lib.GRIDOPS_HEADER)
    assert set(mine) == ENTRIES and all(n.startswith("mf_gridops_") for n in mine)
    for n, (_, _, argnames) in mine.items():
        assert n not in seen, "%s is declared by %s as well" % (n, seen.get(n))
        if n != "mf_gridops_abi_version":
            assert argnames[-1] == "stream", n


def test_the_kernels_are_built_into_the_library():
    from mantaflow_amd import _lib
    csrc = os.path.join(os.path.dirname(_lib.DEFAULT_LIB))
    make = open(os.path.join(csrc, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", make, flags=re.M).group(1).split()
    assert "gridops.hip" in srcs and "-ffp-contract=off" in make
    text = open(os.path.join(csrc, "gridops.hip")).read()
    for n in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
    assert "hipcub" not in text and "rocprim" not in text


def test_cpu_backend_lacks_the_extension(oracle_backend):
    import manta as m
    from mantaflow_amd import _lib
    assert _lib.get().gridops is False
    assert m.Solver(name="o", gridSize=m.vec3(8, 7, 6), dim=3).lib.gridops is False


# ---- a small scene on the CPU backend ---------------------------------------------------------------------------------------------
DIMS = (6, 6, 6)


class Stage(object):
    def __init__(self, m):
        sx, sy, sz = DIMS
        s = self.s = m.Solver(name="o", gridSize=m.vec3(*DIMS), dim=3)
        self.other = m.Solver(name="t", gridSize=m.vec3(*DIMS), dim=3)
        mk = s.create
        self.real, self.real2, self.real3, self.phi = mk(m.RealGrid), mk(m.RealGrid), mk(m.RealGrid), mk(m.LevelsetGrid)
        self.mac, self.mac2, self.vec, self.flags, self.ints = mk(m.MACGrid), mk(m.MACGrid), mk(m.VecGrid), mk(m.FlagGrid), mk(m.IntGrid)
        self.out = self.other.create(m.RealGrid)
        self.noise = mk(m.NoiseField)
        self.grids = dict(real=self.real, real2=self.real2, real3=self.real3, phi=self.phi, mac=self.mac, mac2=self.mac2, vec=self.vec,
                          flags=self.flags, ints=self.ints, out=self.out)
        rng = np.random.RandomState(5)
        for g in (self.real, self.real2, self.real3, self.phi, self.out):
            g.from_numpy((rng.rand(sz, sy, sx) - 0.5).astype(f32))
        for g in (self.mac, self.mac2, self.vec):
            g.from_numpy(rng.rand(sz, sy, sx, 3).astype(f32))
        self.flags.from_numpy(rng.randint(1, 4, (sz, sy, sx)).astype(np.int32))
        self.ints.from_numpy(rng.randint(-9, 9, (sz, sy, sx)).astype(np.int32))

    def snapshot(self):
        snap = {k: g.to_numpy().copy() for k, g in self.grids.items()}
        snap["live"] = (self.s._live, self.other._live)
        snap["pooled"] = {k: len(v) for k, v in self.s._pool.items()}
        return snap

    def unchanged(self, snap):
        now = self.snapshot()
        for k in snap:
            assert np.array_equal(now[k], snap[k]) if isinstance(snap[k], np.ndarray) else now[k] == snap[k], k


def calls(m, S):
    """name -> calls with good arguments and with bad ones: the refusals come before every check"""
    return {
        "Grid::permuteAxes": (lambda: S.real.permuteAxes(1, 0, 2), lambda: S.vec.permuteAxes(2, 1, 0), lambda: S.ints.permuteAxes(0, 0, 7)),
        "Grid::permuteAxesCopyToGrid": (lambda: S.real.permuteAxesCopyToGrid(1, 0, 2, S.out), lambda: S.flags.permuteAxesCopyToGrid(0, 1, 2, out=None)),
        "Grid::getL1": (lambda: S.real.getL1(), lambda: S.mac.getL1(1), lambda: S.flags.getL1(bnd=-1)),
        "Grid::getL2": (lambda: S.ints.getL2(), lambda: S.vec.getL2(bnd=2)),
        "Grid::join": (lambda: S.real.join(S.real2), lambda: S.vec.join(S.mac, False), lambda: S.ints.join(S.real)),
        "addForceField": (lambda: m.addForceField(S.flags, S.mac, S.vec), lambda: m.addForceField(S.flags, S.mac, S.vec, S.real, True),
                          lambda: m.addForceField(S.real, S.mac, S.vec)),
        "setForceField": (lambda: m.setForceField(S.flags, S.mac, S.vec), lambda: m.setForceField(S.flags, S.mac, force=S.real)),
        "setInitialVelocity": (lambda: m.setInitialVelocity(S.flags, S.mac, S.vec), lambda: m.setInitialVelocity(S.flags, S.vec, S.vec)),
        "extrapolateVec3Simple": (lambda: m.extrapolateVec3Simple(S.vec, S.phi), lambda: m.extrapolateVec3Simple(S.vec, S.flags, 2, True)),
        "applyEmission": (lambda: m.applyEmission(S.flags, S.real, S.real2), lambda: m.applyEmission(S.flags, S.real, S.real2, S.real3, False, 8),
                          lambda: m.applyEmission(S.flags, S.real, S.vec)),
        "resetInObstacle": (lambda: m.resetInObstacle(S.flags, S.mac, S.real), lambda: m.resetInObstacle(S.flags, S.mac, None, fuel=S.real2)),
        "copyMACData": (lambda: m.copyMACData(S.mac, S.mac2, S.flags, 1, 0), lambda: m.copyMACData(S.mac, S.vec, S.flags, 1, -1)),
        "copyRealToVec3": (lambda: m.copyRealToVec3(S.real, S.real2, S.real3, S.vec), lambda: m.copyRealToVec3(S.real, S.real2, S.vec, S.vec)),
        "copyVec3ToReal": (lambda: m.copyVec3ToReal(S.vec, S.real, S.real2, S.real3), lambda: m.copyVec3ToReal(S.real, S.real, S.real2, S.real3)),
        "resampleMacToVec3": (lambda: m.resampleMacToVec3(S.mac, S.vec), lambda: m.resampleMacToVec3(S.mac, S.mac)),
        "swapComponents": (lambda: m.swapComponents(S.vec, 2, 2, 0), lambda: m.swapComponents(S.vec, 0, 1, 5)),
        "getGridAvg": (lambda: m.getGridAvg(S.real), lambda: m.getGridAvg(S.real, S.flags), lambda: m.getGridAvg(S.vec)),
        "debugIntToReal": (lambda: m.debugIntToReal(S.ints, S.real), lambda: m.debugIntToReal(S.real, S.real, 2.0)),
        "applySimpleNoiseReal": (lambda: m.applySimpleNoiseReal(S.flags, S.real, S.noise), lambda: m.applySimpleNoiseReal(S.flags, S.real, None, 2.0, S.real2)),
        "applySimpleNoiseVec3": (lambda: m.applySimpleNoiseVec3(S.flags, S.vec, S.noise), lambda: m.applySimpleNoiseVec3(S.flags, S.real, S.noise)),
        "flipComputePotentialTrappedAir": (lambda: m.flipComputePotentialTrappedAir(S.real, S.flags, S.mac, 1, 0.1, 1.0, 0.1),
                                           lambda: m.flipComputePotentialTrappedAir(S.real, S.flags, S.vec, 99, 0.1, 1.0, 0.1, 1, 4)),
        "flipComputePotentialKineticEnergy": (lambda: m.flipComputePotentialKineticEnergy(S.real, S.flags, S.mac, 0.1, 1.0, 0.1),
                                              lambda: m.flipComputePotentialKineticEnergy(S.vec, S.flags, S.mac, 0.1, 1.0, 0.1, itype=5)),
        "flipComputePotentialWaveCrest": (lambda: m.flipComputePotentialWaveCrest(S.real, S.flags, S.mac, 1, S.vec, 0.1, 1.0, 0.1),
                                          lambda: m.flipComputePotentialWaveCrest(S.real, S.flags, S.mac, 1, None, 0.1, 1.0, 0.1)),
        "flipComputeSurfaceNormals": (lambda: m.flipComputeSurfaceNormals(S.vec, S.phi), lambda: m.flipComputeSurfaceNormals(S.real, S.phi)),
        "flipUpdateNeighborRatio": (lambda: m.flipUpdateNeighborRatio(S.flags, S.real, 1), lambda: m.flipUpdateNeighborRatio(S.flags, S.vec, -1, 1, 2)),
    }


KERNEL_BACKED = ["Grid::permuteAxes", "Grid::permuteAxesCopyToGrid", "Grid::getL1", "Grid::getL2", "Grid::join", "addForceField", "setForceField",
                 "setInitialVelocity", "extrapolateVec3Simple", "applyEmission", "resetInObstacle", "copyMACData", "copyRealToVec3",
                 "copyVec3ToReal", "resampleMacToVec3", "swapComponents", "getGridAvg", "debugIntToReal", "applySimpleNoiseReal",
                 "applySimpleNoiseVec3", "flipComputePotentialTrappedAir", "flipComputePotentialKineticEnergy",
                 "flipComputePotentialWaveCrest", "flipComputeSurfaceNormals", "flipUpdateNeighborRatio"]


@pytest.mark.parametrize("name", KERNEL_BACKED)
def test_refused_on_the_cpu_backend_and_on_a_z_slab_solver(oracle_backend, name):
    import manta as m
    S = Stage(m)
    snap = S.snapshot()
    assert set(calls(m, S)) == set(KERNEL_BACKED)
    for call in calls(m, S)[name]:
        with pytest.raises(RuntimeError) as err:
            call()
        assert str(err.value) == "%s: the 'oracle' backend does not implement %s (manta_hip_gridops.h)" % (name, WHAT)
        S.unchanged(snap)
        S.s._slab_window = (4, 40)      # what slab.SlabDomain gives the solver of a z-slab: (z offset, global sz)
        try:
            with pytest.raises(RuntimeError) as err:
                call()
            assert str(err.value) == "%s: %s do not run on a z-slab solver" % (name, WHAT)      # the z-slab check comes first
        finally:
            S.s._slab_window = (0, 0)
        S.unchanged(snap)


def test_levelset_join_keeps_its_own_meaning(oracle_backend):
    import manta as m
    S = Stage(m)
    a, b = S.phi.to_numpy(), S.real.to_numpy()
    S.phi.join(S.real)                                              # KnJoin: the minimum, on every backend
    assert np.array_equal(S.phi.to_numpy(), np.minimum(a, b))


# ---- the permutation's argument checks: they need no kernel, so a library that says it has the extension is enough -------------------
class _Recorder(object):
    """stands for a library with the extension: records the calls instead of making them"""
    def __init__(self, lib):
        self._lib, self.made = lib, []

    def __getattr__(self, k):
        return getattr(self._lib, k)

    def call(self, name, *args):
        self.made.append((name,) + args[:7])


def _with_extension(m, dims, dim=None):
    s = m.Solver(name="p", gridSize=m.vec3(*dims), dim=dim or (3 if dims[2] > 1 else 2))
    s.lib = _Recorder(s.lib)
    s.lib.gridops = True
    return s


def test_permutation_refusals(oracle_backend):
    import manta as m
    dims = (7, 5, 3)
    s = _with_extension(m, dims)
    g = s.create(m.RealGrid)
    for ax in M.PERMUTATIONS:
        odims = [0, 0, 0]
        for n in range(3):
            odims[ax[n]] = dims[n]                                  # what the reference's assert accepts
        t = _with_extension(m, tuple(odims))
        out = t.create(m.RealGrid)
        before = len(s.lib.made)
        if M.permute_refusal(dims, tuple(odims), ax) == "outside":
            with pytest.raises(RuntimeError, match=r"^permuteAxesCopyToGrid: a cyclic permutation"):
                g.permuteAxesCopyToGrid(ax[0], ax[1], ax[2], out)
            assert len(s.lib.made) == before
        else:
            g.permuteAxesCopyToGrid(ax[0], ax[1], ax[2], out)
            assert s.lib.made[-1][:8] == ("mf_gridops_permute", 7, 5, 3, ax[0], ax[1], ax[2], 1)
        with pytest.raises(RuntimeError, match="Grids must have same data type!"):
            g.permuteAxesCopyToGrid(ax[0], ax[1], ax[2], t.create(m.IntGrid))
    before = len(s.lib.made)
    with pytest.raises(RuntimeError, match="Permuted grids must have the same dimensions!"):
        g.permuteAxesCopyToGrid(1, 0, 2, s.create(m.RealGrid))
    with pytest.raises(RuntimeError, match="Grid must be cubic!"):
        g.permuteAxes(1, 0, 2)
    for bad in ((0, 0, 1), (0, 1, 3), (-1, 0, 1), (2, 2, 2)):       # silently nothing, as in the reference
        assert g.permuteAxes(*bad) is None and g.permuteAxesCopyToGrid(bad[0], bad[1], bad[2], g) is None
    assert len(s.lib.made) == before and s._live == 1               # no scratch grid is held
    # 2-D: axis 2 must stay
    s2 = _with_extension(m, (6, 6, 1))
    g2 = s2.create(m.RealGrid)
    thin = _with_extension(m, (6, 1, 6), dim=3).create(m.RealGrid)
    with pytest.raises(RuntimeError, match=r"^permuteAxesCopyToGrid: \(0, 2, 1\) moves axis 2 of a 2-D grid"):
        g2.permuteAxesCopyToGrid(0, 2, 1, thin)
    with pytest.raises(RuntimeError, match=r"^permuteAxes: \(2, 1, 0\) moves axis 2 of a 2-D grid"):
        g2.permuteAxes(2, 1, 0)
    assert s2.lib.made == []
    g2.permuteAxes(1, 0, 2)
    assert s2.lib.made[-1][:8] == ("mf_gridops_permute", 6, 6, 1, 1, 0, 2, 1) and s2._live == 1


def test_reset_value_is_a_real_whatever_its_default_is_spelled(oracle_backend):
    """the wrapper types a parameter by an int default; resetValue is exempt, so a fraction reaches the plugin (which refuses here for
    the backend, not for the number), while a true int parameter still refuses a fraction"""
    import manta as m
    S = Stage(m)
    with pytest.raises(RuntimeError, match="does not implement the grid-operation plugins"):
        m.resetInObstacle(S.flags, S.mac, S.real, resetValue=-1.25)
    with pytest.raises(RuntimeError, match="does not implement the grid-operation plugins"):
        m.resetInObstacle(S.flags, S.mac, S.real, None, None, None, None, None, None, 0.5)
    with pytest.raises(RuntimeError, match="argument is not an int"):
        m.swapComponents(S.vec, 0.5, 1, 2)


# ---- host-only names: every backend ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(M.interp_cases()), ids=lambda c: c[0])
def test_get_interpolated_equals_the_reference(oracle_backend, case):
    import manta as m
    key, dims, kind = case
    s = m.Solver(name="i", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)
    a, pos = M.interp_input(dims, kind), M.interp_positions(dims)
    g = s.create({"real": m.RealGrid, "vec": m.VecGrid, "mac": m.MACGrid}[kind])
    g.from_numpy(a)
    want = GOLDEN[key]
    assert M.same(M.interpolate(a, pos, kind == "mac"), want)                  # the model, every position
    outside = ((pos < 0) | (pos >= np.array(dims, f32))).any(axis=1)
    assert outside.any() and (~outside).any()                                  # both sides of every clamp are in the positions
    for q, p in enumerate(pos):
        got = g.getInterpolated(m.vec3(float(p[0]), float(p[1]), float(p[2])))
        got = np.array([got], f32)[0] if kind == "real" else np.array(list(got), f32)
        assert M.same(got, want[q]), (q, p, got, want[q])
    assert M.same(g.to_numpy(), a)
    for bad in ((float("nan"), 1, 1), (1, float("inf"), 1), (1, 1, -3e10)):
        with pytest.raises(RuntimeError, match="cannot be truncated"):
            g.getInterpolated(m.vec3(*bad))
    if dims[2] == 1 and kind == "mac":
        with pytest.raises(RuntimeError, match="out of bound"):                # interpolMAC multiplies zi by size.y: it leaves the plane
            g.getInterpolated(m.vec3(2.5, 2.5, dims[1] * 3.0))
    elif dims[2] == 1:
        # interpol<T> multiplies zi by the z stride, 0 in 2-D: any z reads the one plane, twice, with weights that sum to 1
        up, here = g.getInterpolated(m.vec3(2.5, 2.5, 7.25)), g.getInterpolated(m.vec3(2.5, 2.5, 0.5))
        assert np.allclose(list(up) if kind == "vec" else up, list(here) if kind == "vec" else here, rtol=1e-6, atol=1e-6)


def test_get_interpolated_on_a_levelset_grid_and_at_cell_centres(oracle_backend):
    import manta as m
    dims = M.SMALL_DIMS[0]
    s = m.Solver(name="i", gridSize=m.vec3(*dims), dim=3)
    a = M.interp_input(dims, "real")
    phi = s.create(m.LevelsetGrid)
    phi.from_numpy(a)
    for (i, j, k) in ((0, 0, 0), (3, 4, 2), (dims[0] - 1, dims[1] - 1, dims[2] - 1)):
        assert f32(phi.getInterpolated(m.vec3(i + 0.5, j + 0.5, k + 0.5))) == a[k, j, i]          # a cell centre is the cell's value


def test_get_npz_file_size(oracle_backend, tmp_path):
    """The recorded reference (built with zlib) returns (0, 0, 0) for a grid file: its guard `#if NO_ZLIB != 1` is inverted.  The package
    returns what the function is written to return, the size in x, y, z order."""
    import manta as m
    assert tuple(GOLDEN["npzsize/file"]) == (0.0, 0.0, 0.0)
    s = m.Solver(name="z", gridSize=m.vec3(*M.NPZ_DIMS), dim=3)
    g = s.create(m.RealGrid)
    g.from_numpy(M.real(M.NPZ_DIMS, "npz"))
    name = str(tmp_path / "g.npz")
    g.save(name)
    size = m.getNpzFileSize(name)
    assert isinstance(size, m.vec3) and tuple(size) == tuple(float(v) for v in M.NPZ_DIMS)
    v = s.create(m.VecGrid)
    v.save(str(tmp_path / "v.npz"))
    assert tuple(m.getNpzFileSize(str(tmp_path / "v.npz"))) == tuple(float(x) for x in M.NPZ_DIMS)
    with pytest.raises(RuntimeError, match="Unable to open file"):
        m.getNpzFileSize(str(tmp_path / "none.npz"))
    np.savez(str(tmp_path / "flat.npz"), arr_0=np.zeros(5, f32))
    with pytest.raises(RuntimeError, match="has 1 dimensions"):
        m.getNpzFileSize(str(tmp_path / "flat.npz"))
    np.savez(str(tmp_path / "other.npz"), data=np.zeros((2, 2, 2), f32))
    with pytest.raises(RuntimeError, match="holds no arr_0"):
        m.getNpzFileSize(str(tmp_path / "other.npz"))


def test_transform_positions_refuses_an_empty_old_size(oracle_backend):
    import manta as m
    s = m.Solver(name="h", gridSize=m.vec3(8, 8, 8), dim=3)
    pp = s.create(m.BasicParticleSystem)
    pos = np.ones((3, 3), f32)
    pp.set_positions(pos, np.zeros(3, np.int32))
    with pytest.raises(RuntimeError, match="not positive"):
        pp.transformPositions(m.vec3(8, 0, 8), m.vec3(16, 16, 16))
    assert np.array_equal(pp.get_positions(), pos)
def test_host_only_grid_accessors(oracle_backend, capsys, tmp_path):
    import manta as m
    dims = M.SMALL_DIMS[0]
    g = M.name_of(dims)
    s = m.Solver(name="h", gridSize=m.vec3(*dims), dim=3)
    src = M.vec(dims, "macsrc")
    mac = s.create(m.MACGrid)
    mac.from_numpy(src)
    # getCentered against the reference's resampleMacToVec3 (the same expression), cell by cell
    want = GOLDEN["resample/" + g]
    for (i, j, k) in ((1, 1, 1), (3, 2, 4), (dims[0] - 2, dims[1] - 2, dims[2] - 2)):
        got = mac.getCentered(m.vec3(i, j, k))
        assert np.array_equal(np.array(list(got), f32), want[k, j, i]), (i, j, k)
        x = mac.getAtMACX(i, j, k)
        assert f32(x.x) == src[k, j, i, 0]
        assert f32(x.y) == f32(0.25) * (src[k, j, i, 1] + src[k, j, i - 1, 1] + src[k, j + 1, i, 1] + src[k, j + 1, i - 1, 1])
        assert f32(x.z) == f32(0.25) * (src[k, j, i, 2] + src[k, j, i - 1, 2] + src[k + 1, j, i, 2] + src[k + 1, j, i - 1, 2])
        y = mac.getAtMACY(i, j, k)
        assert f32(y.y) == src[k, j, i, 1]
        assert f32(y.x) == f32(0.25) * (src[k, j, i, 0] + src[k, j - 1, i, 0] + src[k, j, i + 1, 0] + src[k, j - 1, i + 1, 0])
        z = mac.getAtMACZ(i, j, k)
        assert f32(z.z) == src[k, j, i, 2]
        assert f32(z.y) == f32(0.25) * (src[k, j, i, 1] + src[k - 1, j, i, 1] + src[k, j + 1, i, 1] + src[k - 1, j + 1, i, 1])
    with pytest.raises(RuntimeError, match="out of bound"):
        mac.getCentered(m.vec3(dims[0] - 1, 1, 1))                   # x + 1 is outside
    with pytest.raises(RuntimeError, match="out of bound"):
        mac.getAtMACX(0, 1, 1)
    # get / set
    assert tuple(mac.get(2, 3, 4)) == tuple(float(v) for v in src[4, 3, 2])
    mac.set(2, 3, 4, m.vec3(1.5, -2, 0.25))
    assert tuple(mac.to_numpy()[4, 3, 2]) == (1.5, -2.0, 0.25) and np.array_equal(mac.to_numpy()[4, 3, 3], src[4, 3, 3])
    ints, real = s.create(m.IntGrid), s.create(m.RealGrid)
    ints.set(1, 2, 3, 7)
    real.set(1, 2, 3, 0.1)
    assert ints.get(1, 2, 3) == 7 and isinstance(ints.get(1, 2, 3), int) and f32(real.get(1, 2, 3)) == f32(0.1)
    assert ints.to_numpy().sum() == 7
    for bad in ((-1, 0, 0), (dims[0], 0, 0), (0, dims[1], 0), (0, 0, dims[2])):
        with pytest.raises(RuntimeError, match="out of bound"):
            real.get(*bad)
        with pytest.raises(RuntimeError, match="out of bound"):
            real.set(bad[0], bad[1], bad[2], 1.0)
    # names and the 4-D compatibility accessors
    real.set_name("density")
    assert real.get_name() == real.getName() == "density" and real.getSizeT() == 1 and real.getStrideT() == 0
    # particle positions
    pp = s.create(m.BasicParticleSystem)
    pos = (np.random.RandomState(3).rand(7, 3) * 5).astype(f32)
    pp.set_positions(pos, np.arange(7, dtype=np.int32))
    pp.transformPositions(m.vec3(9, 8, 7), m.vec3(18, 24, 7))
    fac = np.array([f32(18) / f32(9), f32(24) / f32(8), f32(7) / f32(7)], f32)
    assert np.array_equal(pp.get_positions(), pos * fac[None, :]) and np.array_equal(pp.get_flags(), np.arange(7))
    # the uni header printer
    name = str(tmp_path / "d.uni")
    real.save(name)
    capsys.readouterr()
    m.printUniFileInfoString(name)
    assert capsys.readouterr().out.strip() == "File '%s' info: %d,%d,%d" % ((name,) + dims)
    m.printUniFileInfoString(str(tmp_path / "none.uni"))
    assert capsys.readouterr().out.strip().endswith("info: 0,0,0")
