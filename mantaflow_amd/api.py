"""Everything a scene gets from `from manta import *` (reference: module "manta", pwrapper/registry.cpp:390-421,
495-608, plus the constants of source/python/defines.py)."""
import sys

from .core import (BasicParticleSystem, FlagGrid, FluidSolver, Grid, Grid4d, Grid4dBase, Grid4Int, Grid4Real, Grid4Vec3, Grid4Vec4, IntGrid, LevelsetGrid, MACGrid, Mesh, ParticleIndexSystem,
                   PdataInt, PdataReal, PdataVec3, RealGrid, Solver, TurbulenceParticleSystem, Vec3Grid, VecGrid, VortexParticleSystem, resetMovingObstacleState, resetTurbulenceParticleState,
                   resetVortexSeedStream, vec3, vec4)
from .plugins import (Timings, cgSolveDiffusion, getComponent, setComponent, resetOutflow, apicMapPartsToMAC, apicMapMACGridToParts, extrapolateMACFromWeight, extrapolateMACSimple, markFluidCells, addBuoyancy, addGravity, addGravityNoScale, advectSemiLagrange, computePressureRhs,
                      correctVelocity, flipVelocityUpdate, lastCgStats, mapGridToParts, mapGridToPartsVec3, mapMACToParts,
                      mapPartsToGrid, mapPartsToGridVec3, mapPartsToMAC, setDeterministicP2G, setWallBcs, solvePressure,
                      solvePressureSystem, pushOutofObs, gridParticleIndex, unionParticleLevelset, extrapolateLsSimple,
                      setPartType, markIsolatedFluidCell, addForcePvel, updateVelocityFromDeltaPos, eulerStep,
                      interpolateGrid, interpolateGridVec3, interpolateMACGrid, computeEnergy, computeWaveletCoeffs,
                      vorticityConfinement, applyNoiseVec3, setOpenBound,
                      updateFractions, setObstacleFlags, setInflowBcs, addNoise, releaseMG,
                      adjustNumber, combineGridVel,
                      copyFlagsToFlags, markFluidAndBoundaryCells, mapMassToGrid, computeDeltaX, mapMACToPartPositions,
                      averagedParticleLevelset, improvedParticleLevelset,
                      flipComputeSecondaryParticlePotentials, flipSampleSecondaryParticles, flipUpdateSecondaryParticles,
                      flipDeleteParticlesInObstacle, setFlagsFromLevelset, setMACFromLevelset, resetSecondaryParticleStreams,
                      KEpsilonComputeProduction, KEpsilonSources, KEpsilonBcs, KEpsilonGradientDiffusion, computeStrainRateMag,
                      computeVorticity, getCurl,
                      processBurn, updateFlame, calcSecDeriv2d, totalSum, normalizeSumTo, cgSolveWE, resetUvGrid, updateUvWeight,
                      getUvWeight, extrapolateSimpleFlags, initVortexVelocity,
                      PD_fluid_guiding, releaseBlurPrecomp, lastGuidingStats, getSpiralVelocity, setGradientYWeight,
                      densityInflowMesh, densityInflowMeshNoise, lastMeshSdfStats, lastReinitStats,
                      getComp4d, setComp4d, grid4dMaxDiff, grid4dMaxDiffInt, grid4dMaxDiffVec3, grid4dMaxDiffVec4, setRegion4d,
                      setRegion4dVec4, getSliceFrom4d, getSliceFrom4dVec, interpolateGrid4d, interpolateGrid4dVec,
                      setNoisePdata, setNoisePdataVec3, setNoisePdataInt, addTestParts, checkSymmetry, checkSymmetryVec3, testInitGridWithPos,
                      VPseedK41, markAsFixed, densityFromLevelset, smoothMesh, killSmallComponents, lastMeshOpsStats,
                      copyArrayToGridReal, copyGridToArrayReal, copyArrayToGridFlag, copyGridToArrayFlag, copyArrayToGridLevelset,
                      copyGridToArrayLevelset, copyArrayToGridVec3, copyGridToArrayVec3, copyArrayToGridMAC, copyGridToArrayMAC,
                      copyArrayToPdataInt, copyPdataToArrayInt, copyArrayToPdataReal, copyPdataToArrayReal, copyArrayToPdataVec3,
                      copyPdataToArrayVec3, extractFeatureVel, extractFeaturePhi, extractFeatureGeo, getRegions, getRegionalCounts,
                      extendRegion, markSmallRegions, simpleNumpyTest,
                      blurMacGrid, blurRealGrid, calcCenterOfMass, projectImage, projectPpmFull, getLaplacian, getCurvature,
                      set_wall_bcs2, resetPhiInObs,
                      addForceField, setForceField, setInitialVelocity, extrapolateVec3Simple, applyEmission, resetInObstacle, copyMACData,
                      copyRealToVec3, copyVec3ToReal, resampleMacToVec3, swapComponents, getGridAvg, debugIntToReal,
                      applySimpleNoiseReal, applySimpleNoiseVec3,
                      flipComputePotentialTrappedAir, flipComputePotentialKineticEnergy, flipComputePotentialWaveCrest,
                      flipComputeSurfaceNormals, flipUpdateNeighborRatio)

from .scene import (Box, Checkbox, Cylinder, Gui, MovingObstacle, NoiseField, Shape, Slider, Sphere, densityInflow, sampleFlagsWithParticles,
                    sampleLevelsetWithParticles, sampleShapeWithParticles)

WaveletNoiseField = NoiseField     # the class's C++ name; Python scenes of the reference use either (noisefield.h)

# module constants, registry.cpp:390-421
GUI = False
DEBUG = False
MT = True
DOUBLEPRECISION = False
CUDA = False
args = sys.argv[1:]
SCENEFILE = sys.argv[0] if sys.argv else ""

# python/defines.py:25-60
FlagFluid, FlagObstacle, FlagEmpty, FlagInflow, FlagOutflow, FlagStick, FlagReserved = 1, 2, 4, 8, 16, 64, 256
TypeFluid, TypeObstacle, TypeEmpty, TypeInflow, TypeOutflow, TypeStick, TypeReserved = 1, 2, 4, 8, 16, 64, 256
IntEuler, IntRK2, IntRK4 = 0, 1, 2
PcNone, PcMIC, PcMGDynamic, PcMGStatic = 0, 1, 2, 3
PtypeSpray, PtypeBubble, PtypeFoam, PtypeTracer = 2, 4, 8, 16
Compression_None, Compression_Zip, Compression_Blosc = 0, 1, 2

_debug_level = 1


def setDebugLevel(level=1):
    """fluidsolver.cpp:217-223"""
    global _debug_level
    _debug_level = int(level)


def mantaMsg(out, level=1):
    """fluidsolver.cpp:210-212"""
    if level <= _debug_level:
        print(out)


def getUniFileSize(name):
    """fileio/iogrids.cpp:323-371: the grid size in the header of a .uni grid file, (0, 0, 0) where the file cannot be read"""
    import struct
    from . import fileio
    try:
        with fileio.Reader(name) as f:
            ident, head = f.magic(), f.payload(12)
    except OSError:
        return vec3(0, 0, 0)
    if ident not in (b"MNT2", b"M4T2", fileio.GRID, fileio.GRID4D) or len(head) != 12:
        return vec3(0, 0, 0)
    return vec3(*[float(v) for v in struct.unpack("<3i", head)])


def printUniFileInfoString(name):
    """fileio/iogrids.cpp:374-380: prints "File '<name>' info: x,y,z" with ",t" appended for a 4-D grid file; a file that cannot be read
    prints 0,0,0.  (A legacy M4T2 file prints without its fourth dimension here.)"""
    from . import fileio
    size = getUniFileSize(name)
    info = "%d,%d,%d" % (size.x, size.y, size.z)
    try:
        with fileio.Reader(name) as f:
            ident = f.magic()
            if ident in (fileio.GRID, fileio.GRID4D):
                dimt = f.header(ident, "can't read file, no header present")[6]
                if dimt > 0:
                    info += ",%d" % dimt
    except (OSError, RuntimeError):
        pass
    mantaMsg("File '%s' info: %s" % (name, info), 1)


def getNpzFileSize(name):
    """fileio/iogrids.cpp:952-975: the grid size in a .npz grid file, (x, y, z) = (shape[2], shape[1], shape[0]) of its arr_0.  That
    is what the function is written to return and does return in a build without zlib; in a build WITH zlib its guard is inverted
    (`#if NO_ZLIB != 1` prints "file format not supported without zlib" and returns), so the recorded reference gives (0, 0, 0) for
    every file (tests/golden/gridops.npz, npzsize/file).  Here the size is returned.  A file that cannot be opened raises, as
    cnpy::npz_load does; a file without a 3-D arr_0 raises where the reference reads outside the shape."""
    import numpy as np
    try:
        with np.load(name) as z:
            if "arr_0" not in z.files:
                raise RuntimeError("getNpzFileSize: '%s' holds no arr_0" % name)
            shape = z["arr_0"].shape
    except (OSError, ValueError) as e:
        raise RuntimeError("npz_load: Error! Unable to open file %s! (%s)" % (name, e))
    if len(shape) < 3:
        raise RuntimeError("getNpzFileSize: arr_0 of '%s' has %d dimensions, a grid has at least 3" % (name, len(shape)))
    return vec3(float(shape[2]), float(shape[1]), float(shape[0]))


def printBuildInfo():
    from . import fileio
    s = fileio.INFO.decode()
    print(s)
    return s


# python/defines.py:14-22
Real = float
false, true = False, True
Vec3 = vec3
Vec4 = vec4


def assertNumpy():
    """fluidsolver.cpp:226-232 (the numpy bridge is always there)"""


# ---- helpers of the reference's regression harness (tools/tests/helperInclude.py) --------------------------------------
# Host-side comparisons of whole grids / pdata (grid.cpp:437-478, 511-536, initplugins.cpp:297-330): not on the hot path.
def gridMaxDiff(g1, g2):
    """max |g1 - g2|, the difference formed in fp32 (grid.cpp:437-444)"""
    g1.parent.sync()
    return float((g1.data - g2.data).abs().max().item()) if g1.data.numel() else 0.0


def gridMaxDiffInt(g1, g2):
    g1.parent.sync()
    return float((g1.data.double() - g2.data.double()).abs().max().item()) if g1.data.numel() else 0.0


def gridMaxDiffVec3(g1, g2):
    """max over cells of the fp64 sum of component differences (grid.cpp:453-469)"""
    g1.parent.sync()
    n = g1.n
    d = (g1.data.double() - g2.data.double()).abs()
    return float((d[:n] + d[n:2 * n] + d[2 * n:3 * n]).max().item()) if n else 0.0


def copyMacToVec3(source, target):
    """grid.cpp:470-478 (both are SoA Vec3 storage here)"""
    target.copyFrom(source)


convertMacToVec3 = copyMacToVec3


def copyLevelsetToReal(source, target):
    """grid.cpp:511-536"""
    target.copyFrom(source)


convertLevelsetToReal = copyLevelsetToReal


def pdataMaxDiff(a, b):
    """initplugins.cpp:297-330"""
    if type(a) is not type(b):
        raise RuntimeError("pdataMaxDiff problem - different pdata types!")
    if a.size() != b.size():
        raise RuntimeError("pdataMaxDiff problem - different pdata sizes!")
    n = a.size()
    if n == 0:
        return 0.0
    a.parent.sync()
    comps = [(a.data[c * a.cap:c * a.cap + n].double() - b.data[c * b.cap:c * b.cap + n].double()).abs() for c in range(a._ncomp)]
    d = comps[0]
    for c in comps[1:]:
        d = d + c
    return float(d.max().item())
