"""CPU: the public face of surface turbulence without a GPU -- the opt-in module and its four names with the reference's signature,
the absence of the names from `manta`, the row of the open extension table with its header, entry names disjoint from every other
extension, the host entries of the built library against the recorded reference (parameters, list resolutions), and the refusals by
name (the CPU checker backend, a z-slab solver, wrong arguments) with every system and the process-wide state left as they were.
The 2-D refusal comes after those two and is checked in tests/test_gpu_surfturb.py with the kernels."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest

import surfturb_model as M
import util

f32 = np.float32


def test_names_are_opt_in_and_signatures():
    import manta
    from mantaflow_amd import api, surfturb
    for n in ("particleSurfaceTurbulence", "debugCheckParts", "resetSurfaceTurbulenceState", "lastSurfaceTurbulenceStats"):
        assert not hasattr(manta, n) and not hasattr(api, n), n
        assert n in surfturb.__all__ and callable(getattr(surfturb, n))
    assert str(inspect.signature(surfturb.particleSurfaceTurbulence)) == (
        "(flags, coarseParts, coarsePartsPrevPos, surfPoints, surfaceNormals, surfaceWaveH, surfaceWaveDtH, surfacePointsDisplaced, "
        "surfaceWaveSource, surfaceWaveSeed, surfaceWaveSeedAmplitude, res, outerRadius=1.0, surfaceDensity=20, nbSurfaceMaintenanceIterations=4, "
        "dt=0.005, waveSpeed=16.0, waveDamping=0.0, waveSeedFrequency=4, waveMaxAmplitude=0.25, waveMaxFrequency=800, waveMaxSeedingAmplitude=0.5, "
        "waveSeedingCurvatureThresholdRegionCenter=0.025, waveSeedingCurvatureThresholdRegionRadius=0.01, waveSeedStepSizeRatioOfMax=0.05)")
    assert str(inspect.signature(surfturb.debugCheckParts)) == "(parts, flags)"
    assert str(inspect.signature(surfturb.resetSurfaceTurbulenceState)) == "()"
    assert str(inspect.signature(surfturb.lastSurfaceTurbulenceStats)) == "()" and isinstance(surfturb.lastSurfaceTurbulenceStats(), dict)
    g = {}
    exec("from mantaflow_amd.surfturb import *\nfrom manta import *", g)       # how a scene gets the plugin
    assert g["particleSurfaceTurbulence"] is surfturb.particleSurfaceTurbulence and "Solver" in g


def test_row_of_the_open_table_and_header():
    from mantaflow_amd import _lib
    e = _lib.extension("surfturb")
    assert e in _lib.OPEN_EXTENSIONS and (e.what, e.verb) == ("surface turbulence", "does")
    inc = os.path.dirname(_lib.HEADER)
    assert e.header == os.path.join(inc, "open", "manta_hip_surfturb.h") == _lib.SURFTURB_HEADER and os.path.exists(e.header)
    assert {x.header for x in _lib.OPEN_EXTENSIONS} == set(glob.glob(os.path.join(inc, "open", "manta_hip_*.h")))
    assert (e.version_fn, e.version_macro) == ("mf_surfturb_abi_version", "MF_SURFTURB_ABI_VERSION")
    assert re.search(r"^#define\s+MF_SURFTURB_ABI_VERSION\s+\d+\s*$", open(e.header).read(), flags=re.M)
    restype, argtypes, _ = _lib.parse_header(e.header)[e.version_fn]
    assert restype is ctypes.c_int and argtypes == []


def test_entry_names_are_disjoint_from_every_other_header():
    from mantaflow_amd import _lib
    seen = {n: "manta_hip.h" for n in _lib.parse_header()}
    for e in _lib.all_extensions():
        if e.name != "surfturb":
            for n in _lib.parse_header(e.header):
                seen[n] = os.path.basename(e.header)
    mine = _lib.parse_header(_lib.SURFTURB_HEADER)
    assert len(mine) == 21 and all(n.startswith("mf_surfturb_") for n in mine)
    for n in mine:
        assert n not in seen, "%s is declared by %s as well" % (n, seen.get(n))


@pytest.mark.skipif(not os.path.exists(util.HIP_LIB), reason="libmanta_hip.so not built")
def test_host_entries_of_the_product_library_equal_the_recorded_reference():
    from mantaflow_amd import _lib
    L = ctypes.CDLL(util.HIP_LIB)          # loads without a GPU; only the host entries are called
    for n in _lib.parse_header(_lib.SURFTURB_HEADER):
        assert hasattr(L, n), n
    G = M.golden()
    fc = ctypes.c_float
    for k in range(3):
        a = G["set%d/args" % k]
        par, rr = (fc * 32)(), (ctypes.c_int32 * 2)()
        assert L.mf_surfturb_params(M.RES, fc(a[0]), int(a[1]), *([fc(x) for x in a[3:]] + [0, par, rr])) == 0
        assert np.array(list(par)[:9], f32).tobytes() == G["set%d/par" % k].tobytes(), k
        assert list(rr) == G["set%d/res" % k].tolist()
        count = ctypes.c_int64(0)
        assert L.mf_surfturb_directions(par, ctypes.c_int64(0), None, ctypes.byref(count)) == 0
        dirs = np.zeros((count.value, 3), f32)
        assert L.mf_surfturb_directions(par, count, dirs.ctypes.data_as(ctypes.c_void_p), ctypes.byref(count)) == 0
        assert count.value == {0: 53, 1: 137, 2: 79}[k] and np.allclose(np.linalg.norm(dirs.astype(np.float64), axis=1), 1, atol=1e-6)
        assert dirs[0].tolist() == [0.0, 1.0, 0.0]
    assert L.mf_surfturb_params(3, fc(1), 20, *([fc(0)] * 10 + [0, par, rr])) != 0
    need = ctypes.c_int64(0)
    L.mf_surfturb_tmp_bytes.argtypes = [ctypes.c_int64] * 3 + [ctypes.c_void_p]
    assert L.mf_surfturb_tmp_bytes(1000, 27000, 1000, ctypes.byref(need)) == 0 and need.value >= 16 * 1000
    assert L.mf_surfturb_tmp_bytes(-1, 5, 0, ctypes.byref(need)) != 0


def _scene(m, dim=3):
    s = m.Solver(name="o", gridSize=m.vec3(12, 12, 12 if dim == 3 else 1), dim=dim)
    flags = s.create(m.FlagGrid)
    flags.initDomain(boundaryWidth=1)
    pp, sp, spd = (s.create(m.BasicParticleSystem) for _ in range(3))
    prev = pp.create(m.PdataVec3)
    ch = [sp.create(m.PdataVec3)] + [sp.create(m.PdataReal) for _ in range(5)]
    pp.set_positions(np.array([[5, 5, 0.5 if dim == 2 else 5], [5.5, 5, 0.5 if dim == 2 else 5]], f32))
    sp.set_positions(np.array([[5, 6, 0.5 if dim == 2 else 5]], f32))
    args = dict(flags=flags, coarseParts=pp, coarsePartsPrevPos=prev, surfPoints=sp, surfaceNormals=ch[0], surfaceWaveH=ch[1], surfaceWaveDtH=ch[2],
                surfacePointsDisplaced=spd, surfaceWaveSource=ch[3], surfaceWaveSeed=ch[4], surfaceWaveSeedAmplitude=ch[5], res=12)
    return s, args


def _snapshot(args):
    from mantaflow_amd import surfturb
    out = [surfturb._state.frameCount, surfturb._state.Rc, surfturb._state.Rs]
    for k in ("coarseParts", "surfPoints", "surfacePointsDisplaced"):
        p = args[k]
        out += [p.np, p.cap, p.mDeletes, p.mDeleteChunk, p.get_positions().tobytes(), p.get_flags().tobytes()]
    return out


def test_refusals_name_the_plugin_and_touch_nothing(oracle_backend):
    import manta as m
    from mantaflow_amd import surfturb
    surfturb.resetSurfaceTurbulenceState()
    s, args = _scene(m)
    before = _snapshot(args)
    with pytest.raises(RuntimeError) as e:
        surfturb.particleSurfaceTurbulence(**args)
    assert str(e.value) == "particleSurfaceTurbulence: the 'oracle' backend does not implement surface turbulence (manta_hip_surfturb.h)"
    with pytest.raises(RuntimeError) as e:
        surfturb.debugCheckParts(args["coarseParts"], args["flags"])
    assert str(e.value) == "debugCheckParts: the 'oracle' backend does not implement surface turbulence (manta_hip_surfturb.h)"
    s._slab_window = (2, 8)
    try:
        for who, call in (("particleSurfaceTurbulence", lambda: surfturb.particleSurfaceTurbulence(**args)),
                          ("debugCheckParts", lambda: surfturb.debugCheckParts(parts=args["surfPoints"], flags=args["flags"]))):
            with pytest.raises(RuntimeError) as e:
                call()
            assert str(e.value) == who + ": surface turbulence does not run on a z-slab solver"
    finally:
        s._slab_window = (0, 0)
    with pytest.raises(RuntimeError) as e:
        surfturb.particleSurfaceTurbulence(**dict(args, flags=args["coarseParts"]))
    assert str(e.value) == "can't convert argument to FlagGrid*"
    with pytest.raises(RuntimeError, match="argument is not an int"):
        surfturb.particleSurfaceTurbulence(**dict(args, surfaceDensity=12.5))
    with pytest.raises(RuntimeError, match="Argument .* unknown"):
        surfturb.particleSurfaceTurbulence(**dict(args, waveSped=3.0))
    assert _snapshot(args) == before
    assert surfturb.lastSurfaceTurbulenceStats() == {}
