"""Python-callable operators ("plugins") of the hot path, same names / parameter order / defaults as the reference's
PYTHON() declarations; orchestration mirrors the reference function by function, arithmetic happens in the C ABI.

  advectSemiLagrange                         source/plugin/advection.cpp:443-461
  computePressureRhs / solvePressureSystem / correctVelocity / solvePressure   source/plugin/pressure.cpp:277-523
  mapPartsToMAC / mapMACToParts / flipVelocityUpdate / mapPartsToGrid(+Vec3) / mapGridToParts(+Vec3)
                                             source/plugin/flip.cpp:637-742
  setWallBcs / addBuoyancy / addGravity      source/plugin/extforces.cpp (SURVEY 8f-1 glue)
  updateFractions / setObstacleFlags / addNoise   source/plugin/initplugins.cpp:45-51, 351-474
  setWallBcs(fractions=, phiObs=) / setInflowBcs  source/plugin/extforces.cpp:163-182, 240-335
                                             (include/manta_hip_obstacles.h; not on z-slab solvers)
  adjustNumber / combineGridVel              source/plugin/flip.cpp:204-262, 748-776
                                             (include/manta_hip_resample.h; not on z-slab solvers)
  copyFlagsToFlags / markFluidAndBoundaryCells / mapMassToGrid / computeDeltaX / mapMACToPartPositions
                                             source/plugin/implicitdensityprojection.cpp
                                             (include/manta_hip_idp.h; not on z-slab solvers)
  averagedParticleLevelset / improvedParticleLevelset   source/plugin/flip.cpp:365-581
                                             (include/manta_hip_partls.h; not on z-slab solvers)
  PD_fluid_guiding / releaseBlurPrecomp / getSpiralVelocity / setGradientYWeight   source/plugin/fluidguiding.cpp
                                             (include/manta_hip_guiding.h; the solve not on z-slab solvers)
  flipComputeSecondaryParticlePotentials / flipSampleSecondaryParticles / flipUpdateSecondaryParticles /
  flipDeleteParticlesInObstacle / setFlagsFromLevelset / setMACFromLevelset   source/plugin/secondaryparticles.cpp
                                             (include/manta_hip_secparts.h; not on z-slab solvers)
  KEpsilonComputeProduction / KEpsilonSources / KEpsilonBcs / KEpsilonGradientDiffusion   source/plugin/kepsilon.cpp
  computeStrainRateMag / computeVorticity / getCurl   source/plugin/waveletturbulence.cpp:204-236, 310-316
                                             (include/ext/manta_hip_turbulence.h; not on z-slab solvers)
  processBurn / updateFlame                   source/plugin/fire.cpp
  calcSecDeriv2d / totalSum / normalizeSumTo / cgSolveWE   source/plugin/waves.cpp
  resetUvGrid / updateUvWeight / getUvWeight  source/grid.cpp:573-627
  extrapolateSimpleFlags                      source/plugin/waveletturbulence.cpp:239-307
  initVortexVelocity                          source/plugin/initplugins.cpp:478-503
                                             (include/open/manta_hip_fields.h; not on z-slab solvers)
  copyArrayToGrid* / copyGridToArray* / copyArrayToPdata* / copyPdataToArray*   source/plugin/numpyconvert.cpp:145-223
  simpleNumpyTest / extractFeatureVel / extractFeaturePhi / extractFeatureGeo / getRegions / getRegionalCounts / extendRegion /
  markSmallRegions                            source/plugin/tfplugins.cpp
                                             (include/open/manta_hip_mlflip.h; not on z-slab solvers)
  blurMacGrid / blurRealGrid / calcCenterOfMass / projectPpmFull (+ projectImage)   source/plugin/initplugins.cpp:273-282, 337-348, 510-655
  getLaplacian / getCurvature                 source/plugin/flip.cpp:779-785
                                             (include/open/manta_hip_datagen.h; not on z-slab solvers)
  set_wall_bcs2 / resetPhiInObs / extrapolateMACSimple(phiObs=)   source/plugin/extforces.cpp:337-373, advection.cpp:397-402,
                                             fastmarch.cpp:303-375 (include/open/manta_hip_movingobs.h; not on z-slab solvers)
  addForceField / setForceField / setInitialVelocity   source/plugin/extforces.cpp:24-43, 376-407, 430-436
  extrapolateVec3Simple                       source/fastmarch.cpp:525-557
  applyEmission / resetInObstacle             source/plugin/initplugins.cpp:110-128, 154-183
  copyMACData / copyRealToVec3 / copyVec3ToReal / resampleMacToVec3 / swapComponents / getGridAvg / debugIntToReal
                                             source/grid.cpp:496-536, 564-571, 717-739, 1013-1033, plugin/flip.cpp:266-269
  applySimpleNoiseReal / applySimpleNoiseVec3 source/plugin/waveletturbulence.cpp:85-116
  flipComputePotentialTrappedAir / flipComputePotentialKineticEnergy / flipComputePotentialWaveCrest / flipComputeSurfaceNormals /
  flipUpdateNeighborRatio                     source/plugin/secondaryparticles.cpp:549-706
                                             (include/open/manta_hip_gridops.h; not on z-slab solvers)
  smoothMesh / killSmallComponents            source/plugin/meshplugins.cpp:36-104, 563-619
                                             (include/open/manta_hip_meshops.h; not on z-slab solvers)
"""
import ctypes
import functools
import time

import numpy as np
import torch

from . import _lib, core
from .core import (FlagGrid, Grid, GridBase, LevelsetGrid, MACGrid, VecGrid, _extension_lib, _ptr, _to_vec3, vec3)

PcNone, PcMIC, PcMGDynamic, PcMGStatic = 0, 1, 2, 3
IntEuler, IntRK2, IntRK4 = 0, 1, 2

_UNIVERSAL = ("notiming", "parent", "name", "nocheck", "solver")   # codegen_python.cpp:37, pconvert.cpp:461,477
_timings = {}
_last_cg = {}


def _coerce(v, default):
    """fromPy<bool> / fromPy<int>, pconvert.cpp:170-181, 212-215: a bool parameter takes a Python bool only; an int parameter
    takes an int, or a float within 1e-5 of an integer"""
    if isinstance(default, bool):
        if not isinstance(v, bool):
            raise RuntimeError("argument is not a boolean")
        return v
    if isinstance(default, int):
        if isinstance(v, (int, np.integer)):
            return int(v)
        if isinstance(v, (float, np.floating)):
            a = float(v)
            if abs(a - np.floor(a + 0.5)) > 1e-5:
                raise RuntimeError("argument is not an int")
            return int(a + 0.5)
        raise RuntimeError("argument is not an int")
    return v


def plugin(fn):
    """Wrapper every PYTHON() symbol gets in the reference (codegen_python.cpp:32-58): universal kwargs, per-plugin
    wall timer (pclass.cpp:36-41), unknown arguments -> RuntimeError (pconvert.cpp:460-474), bool / int argument conversion
    rules (typed by the parameter's default value)."""
    import inspect
    params = list(inspect.signature(fn).parameters.values())
    typed = {p.name: p.default for p in params if isinstance(p.default, (bool, int)) and p.default is not None
             and p.name not in getattr(fn, "_real_parameters", ())}
    pos_typed = [(i, p.default) for i, p in enumerate(params) if p.name in typed]

    @functools.wraps(fn)
    def w(*args, **kw):
        notiming = kw.pop("notiming", False)
        for k in _UNIVERSAL[1:]:
            kw.pop(k, None)
        if typed:
            if any(i < len(args) for i, _ in pos_typed):
                args = list(args)
                for i, d in pos_typed:
                    if i < len(args):
                        args[i] = _coerce(args[i], d)
            for k in kw:
                if k in typed:
                    kw[k] = _coerce(kw[k], typed[k])
        t0 = time.time()
        try:
            r = fn(*args, **kw)
        except TypeError as e:
            msg = str(e)
            if "unexpected keyword argument" in msg:
                raise RuntimeError("Argument %s unknown" % msg.split("argument")[-1].strip())
            raise RuntimeError(msg)
        if not notiming:
            rec = _timings.setdefault(fn.__name__, [0, 0.0])
            rec[0] += 1
            rec[1] += time.time() - t0
        return r
    return w


def real_parameters(*names):
    """for a plugin whose reference signature spells a Real default as an int literal (`Real resetValue=0`): those parameters are not
    typed by their default, so they take any number.  Goes below @plugin."""
    def mark(fn):
        fn._real_parameters = names
        return fn
    return mark


class Timings(object):
    """TimingData, timing.{h,cpp}: per-plugin wall time (host clock; kernels are asynchronous on the stream)."""
    def display(self):
        for k, (n, t) in sorted(_timings.items(), key=lambda kv: -kv[1][1]):
            print("[%8.3fs] %s (%d calls)" % (t, k, n))
    def saveMean(self, filename):
        with open(filename, "w") as f:
            for k, (n, t) in _timings.items():
                f.write("%s: %f\n" % (k, t / max(n, 1)))
    def step(self): pass


def _chk(obj, cls, what):
    if not isinstance(obj, cls):
        raise RuntimeError("can't convert argument to %s*" % what)
    return obj


def _opt(obj, cls, what):
    if obj is None or (isinstance(obj, int) and obj == 0):   # None or int 0 is NULL (pclass.cpp:128-134)
        return None
    return _chk(obj, cls, what)


# =========================================================================================================
# advection
# =========================================================================================================
@plugin
def advectSemiLagrange(flags, vel, grid, order=1, strength=1.0, orderSpace=1, openBounds=False, boundaryWidth=-1,
                       clampMode=2, orderTrace=1):
    _chk(flags, FlagGrid, "FlagGrid")
    _chk(vel, MACGrid, "MACGrid")
    _chk(grid, GridBase, "GridBase")
    if order not in (1, 2):
        raise RuntimeError("AdvectSemiLagrange: Only order 1 (regular SL) and 2 (MacCormack) supported")
    if orderSpace not in (1, 2):
        raise RuntimeError("Unknown interpolation order %s" % orderSpace)      # getInterpolatedHi, grid.h:157
    s = flags.parent
    lib, st = s.lib, s.stream
    sx, sy, sz = flags.dims
    dt = s.getDt()
    t = grid.getType()
    if t & GridBase.TypeMAC:
        # fnAdvectSemiLagrange<MACGrid>, advection.cpp:407-437
        # (the three temp grids are written in every cell by their kernels -- the semi-Lagrange steps put the zeros of a fresh grid
        # on the border themselves -- so they come from the pool without the constructor's clear)
        fwd = _scratch_grid(s, MACGrid)
        lib.call("mf_semi_lagrange_mac", sx, sy, sz, vel.ptr, fwd.ptr, grid.ptr, dt, int(orderTrace), int(orderSpace), st)
        if order == 1:
            _apply_outflow_bc(flags, fwd, grid, dt)
            grid.swap(fwd)
        else:
            bwd, newg = _scratch_grid(s, MACGrid), _scratch_grid(s, MACGrid)
            lib.call("mf_semi_lagrange_mac", sx, sy, sz, vel.ptr, bwd.ptr, fwd.ptr, -dt, int(orderTrace), int(orderSpace), st)
            # MacCormackCorrectMAC + MacCormackClampMAC, fused (the clamp reads the corrected value of its own cell only)
            lib.call("mf_maccormack_correct_clamp_mac", sx, sy, sz, flags.ptr, vel.ptr, newg.ptr, grid.ptr, fwd.ptr, bwd.ptr, float(strength),
                     dt, int(clampMode), st)
            _apply_outflow_bc(flags, newg, grid, dt)
            grid.swap(newg)
    elif t & (GridBase.TypeReal | GridBase.TypeVec3):
        # fnAdvectSemiLagrange<GridType>, advection.cpp:293-322
        ncomp = 1 if (t & GridBase.TypeReal) else 3
        G = type(grid)
        sl = "mf_semi_lagrange_real" if ncomp == 1 else "mf_semi_lagrange_vec3"
        fwd = _scratch_grid(s, G)
        lib.call(sl, sx, sy, sz, vel.ptr, fwd.ptr, grid.ptr, dt, int(orderTrace), int(orderSpace), st)
        if order == 1:
            grid.swap(fwd)
        else:
            bwd, newg = _scratch_grid(s, G), _scratch_grid(s, G)
            lib.call(sl, sx, sy, sz, vel.ptr, bwd.ptr, fwd.ptr, -dt, int(orderTrace), int(orderSpace), st)
            lib.call("mf_maccormack_correct_clamp", sx, sy, sz, ncomp, flags.ptr, vel.ptr, newg.ptr, grid.ptr, fwd.ptr, bwd.ptr,
                     float(strength), dt, int(clampMode), st)
            grid.swap(newg)
    else:
        raise RuntimeError("AdvectSemiLagrange: Grid Type is not supported (only Real, Vec3, MAC, Levelset)")


def _apply_outflow_bc(flags, vel, velPrev, dt):
    """applyOutflowBC, advection.cpp:388-392 (temp MAC grid so vel is not overwritten while it is read)"""
    s = flags.parent
    if not getattr(flags, "_may_have_outflow", True):
        return
    velDst = MACGrid(s)
    s.lib.call("mf_apply_outflow_bc", flags.sx, flags.sy, flags.sz, flags.ptr, vel.ptr, velPrev.ptr, velDst.ptr, float(dt), s.stream)


# =========================================================================================================
# pressure projection
# =========================================================================================================
@plugin
def computePressureRhs(rhs, vel, pressure, flags, cgAccuracy=1e-3, phi=None, perCellCorr=None, fractions=None, obvel=None,
                       gfClamp=1e-04, cgMaxIterFac=1.5, precondition=True, preconditioner=PcMIC,
                       enforceCompatibility=False, useL2Norm=False, zeroPressureFixing=False, curv=None, surfTens=0.):
    _chk(rhs, Grid, "Grid<Real>"); _chk(vel, MACGrid, "MACGrid"); _chk(flags, FlagGrid, "FlagGrid")
    phi, perCellCorr, curv = _opt(phi, Grid, "Grid<Real>"), _opt(perCellCorr, Grid, "Grid<Real>"), _opt(curv, Grid, "Grid<Real>")
    fractions, obvel = _opt(fractions, MACGrid, "MACGrid"), _opt(obvel, MACGrid, "MACGrid")
    s = flags.parent
    cnt, sm = ctypes.c_int32(0), ctypes.c_double(0.0)
    need = bool(enforceCompatibility)
    s.lib.call("mf_make_rhs", flags.sx, flags.sy, flags.sz, flags.ptr, rhs.ptr, vel.ptr,
               None if perCellCorr is None else perCellCorr.ptr, None if fractions is None else fractions.ptr,
               None if obvel is None else obvel.ptr, None if phi is None else phi.ptr, None if curv is None else curv.ptr,
               float(surfTens), float(gfClamp), ctypes.byref(cnt) if need else None, ctypes.byref(sm) if need else None, s.stream)
    if enforceCompatibility:
        # rhs += (Real)(-kernMakeRhs.sum / (Real)kernMakeRhs.cnt), pressure.cpp:297-298
        corr = np.float32(-sm.value / float(np.float32(cnt.value)))
        rhs.addConst(float(corr))


@plugin
def solvePressureSystem(rhs, vel, pressure, flags, cgAccuracy=1e-3, phi=None, perCellCorr=None, fractions=None, gfClamp=1e-04,
                        cgMaxIterFac=1.5, precondition=True, preconditioner=PcMIC, enforceCompatibility=False,
                        useL2Norm=False, zeroPressureFixing=False, curv=None, surfTens=0.):
    _chk(rhs, Grid, "Grid<Real>"); _chk(vel, MACGrid, "MACGrid"); _chk(pressure, Grid, "Grid<Real>"); _chk(flags, FlagGrid, "FlagGrid")
    phi = _opt(phi, Grid, "Grid<Real>")
    fractions = _opt(fractions, MACGrid, "MACGrid")
    if precondition is False:
        preconditioner = PcNone
    s = flags.parent
    lib, st = s.lib, s.stream
    sx, sy, sz = flags.dims
    if preconditioner in (PcMGDynamic, PcMGStatic):
        _multigrid_lib(s, "solvePressureSystem")
    # reserve temp grids, pressure.cpp:332-338
    residual, search, A0, Ai, Aj, Ak, tmp = (Grid(s) for _ in range(7))
    lib.call("mf_make_laplace_matrix", sx, sy, sz, flags.ptr, A0.ptr, Ai.ptr, Aj.ptr, Ak.ptr,
             None if fractions is None else fractions.ptr, st)
    if phi is not None:
        lib.call("mf_apply_ghost_fluid_diagonal", sx, sy, sz, A0.ptr, flags.ptr, phi.ptr, float(gfClamp), st)
    if zeroPressureFixing or cgAccuracy < 1e-07:
        _fix_pressure(flags, rhs, A0, Ai, Aj, Ak)
    if preconditioner in (PcNone, PcMIC):
        gmax = max(sx, sy, sz)
        maxIter = int(np.float32(cgMaxIterFac) * np.float32(gmax)) * (1 if flags.is3D() else 4)   # pressure.cpp:410
        pca0 = Grid(s)
        pca1, pca2, pca3 = Grid(s), Grid(s), Grid(s)   # allocated (and zeroed) by the reference as well, :412-415
        if preconditioner == PcNone:
            # setICPreconditioner(PC_None, ...) asserts in the reference (conjugategrad.cpp:312); keep the behaviour
            raise RuntimeError("GridCg<APPLYMAT>::setICPreconditioner: Invalid method specified.")
        pc = 2   # PC_mICP ; 2-D degrades to PC_None inside the solver (conjugategrad.cpp:315-321)
    elif preconditioner in (PcMGDynamic, PcMGStatic):
        # pressure.cpp:419-431, 452-454: one GridMg per solver; Dynamic releases an existing one first and its own after the solve,
        # Static keeps it -- with its matrix: a later Static solve preconditions with the old hierarchy, whatever the flags are now
        if s._mg is not None and preconditioner == PcMGDynamic:
            _release_mg(s)
        if s._mg is None:
            s._mg = _MgHandle(lib, sx, sy, sz)
            _mg_solvers.add(s)
        out = (ctypes.c_float * 3)()
        try:
            s._mg.cg_solve((sx, sy, sz), flags, pressure, rhs, residual, search, tmp, (A0, Ai, Aj, Ak), cgAccuracy, 100, useL2Norm, out, st)   # maxIter = 100, :419
        except RuntimeError as e:
            if "diverged" in str(e):
                # conjugategrad.cpp:287-291
                print("GridCg::iterate: Warning - this diverging solve can be caused by the 'static' mode of the MG preconditioner. "
                      "If the static mode is active, try switching to dynamic.")
            raise
        _last_cg["iterations"], _last_cg["residual"] = int(out[0]), float(out[1])
        if preconditioner == PcMGDynamic:
            _release_mg(s)
        return
    else:
        maxIter, pc, pca0 = 0, 0, Grid(s)
    out = (ctypes.c_float * 3)()
    lib.call("mf_cg_solve", sx, sy, sz, flags.ptr, pressure.ptr, rhs.ptr, residual.ptr, search.ptr, tmp.ptr,
             A0.ptr, Ai.ptr, Aj.ptr, Ak.ptr, pca0.ptr, pc, float(cgAccuracy), int(maxIter), int(bool(useL2Norm)), out, st)
    _last_cg["iterations"], _last_cg["residual"] = int(out[0]), float(out[1])


@plugin
def cgSolveDiffusion(flags, grid, alpha=0.25, cgMaxIterFac=1.0, cgAccuracy=1e-4):
    """conjugategrad.cpp:350-423: (I + alpha*L) u = grid, unpreconditioned GridCg<ApplyMatrix/2D>; Vec3 / MAC grids component by
    component (2 components in 2-D)"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(grid, GridBase, "GridBase")
    s = flags.parent
    lib, st = s.lib, s.stream
    sx, sy, sz = flags.dims
    rhs, residual, search, tmp, A0, Ai, Aj, Ak = (Grid(s) for _ in range(8))
    dummy = FlagGrid(s)
    dummy.setConst(core.TypeFluid)
    lib.call("mf_make_laplace_matrix", sx, sy, sz, dummy.ptr, A0.ptr, Ai.ptr, Aj.ptr, Ak.ptr, None, st)
    lib.call("mf_diffusion_matrix", sx, sy, sz, flags.ptr, A0.ptr, Ai.ptr, Aj.ptr, Ak.ptr, float(alpha), st)
    maxIter = int(np.float32(cgMaxIterFac) * np.float32(max(sx, sy, sz))) * (1 if flags.is3D() else 4)
    out = (ctypes.c_float * 3)()
    none = Grid(s)

    def solve(u):
        rhs.copyFrom(u)
        lib.call("mf_cg_solve", sx, sy, sz, flags.ptr, u.ptr, rhs.ptr, residual.ptr, search.ptr, tmp.ptr, A0.ptr, Ai.ptr, Aj.ptr, Ak.ptr,
                 none.ptr, PcNone, float(cgAccuracy), int(maxIter), 1, out, st)   # GridCgInterface() : mUseL2Norm(true), conjugategrad.h:31
        _last_cg["iterations"], _last_cg["residual"] = int(out[0]), float(out[1])

    t = grid.getType()
    if t & GridBase.TypeReal:
        solve(grid)
    elif t & (GridBase.TypeVec3 | GridBase.TypeMAC):
        u = Grid(s)
        for comp in range(3 if grid.is3D() else 2):
            lib.call("mf_copy_f32", u.n, u.ptr, _ptr(grid.data[comp * grid.n:]), st)
            solve(u)
            lib.call("mf_copy_f32", u.n, _ptr(grid.data[comp * grid.n:]), u.ptr, st)
    else:
        raise RuntimeError("cgSolveDiffusion: Grid Type is not supported (only Real, Vec3, MAC, or Levelset)")


class _MgHandle(object):
    """a multigrid hierarchy of the library, destroyed with the object: of manta_hip_multigrid.h on a 3-D grid, of
    open/manta_hip_mg2d.h (the same entries, one for one, without sz and Ak) when sz == 1"""

    def __init__(self, lib, sx, sy, sz):
        self.lib = lib
        self.two_d = sz == 1
        self.prefix = "mf_mg2d_" if self.two_d else "mf_mg_"
        h = ctypes.c_void_p()
        lib.call(self.prefix + "create", *((sx, sy) if self.two_d else (sx, sy, sz)), ctypes.byref(h))
        self.handle = h

    def cg_solve(self, dims, flags, pressure, rhs, residual, search, tmp, A, cgAccuracy, maxIter, useL2Norm, out, st):
        """mf_mg_cg_solve / mf_mg2d_cg_solve on the grids' pointers; A: the four coefficient grids (a 2-D system has no Ak)"""
        size, coef = (dims[:2], A[:3]) if self.two_d else (dims, A)
        self.lib.call(self.prefix + "cg_solve", self.handle, *size, flags.ptr, pressure.ptr, rhs.ptr, residual.ptr, search.ptr, tmp.ptr,
                      *[a.ptr for a in coef], float(cgAccuracy), int(maxIter), int(bool(useL2Norm)), out, st)

    def release(self):
        if self.handle is not None:
            h, self.handle = self.handle, None
            self.lib.call(self.prefix + "destroy", h)

    def info(self):
        """levels, set-ups so far, coarsest-CG iterations of the last V-cycle, per-level sizes and active vertices (mf_mg_info /
        mf_mg2d_info)"""
        out = (ctypes.c_int64 * (8 + 4 * 16))()
        self.lib.call(self.prefix + "info", self.handle, out, len(out))
        nl = int(out[0])
        return dict(levels=nl, setups=int(out[1]), coarse_cg_iterations=int(out[2]), nonzero_stencil_sum=bool(out[3]),
                    trivial_equations=bool(out[4]), tail_first_level=int(out[5]), setup_host_us=int(out[6]), setup_device_us=int(out[7]),
                    sizes=[tuple(int(out[8 + 4 * l + c]) for c in range(3)) for l in range(nl)],
                    active=[int(out[11 + 4 * l]) for l in range(nl)])

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


_mg_solvers = __import__("weakref").WeakSet()    # solvers that hold a hierarchy (gMapMG, pressure.cpp:248)


_multigrid_2d = False    # the process-wide switch of mantaflow_amd.multigrid2d (setMultigrid2D): off unless a scene turns it on


def _multigrid_lib(s, name):
    """refuse, before any grid is touched, what the multigrid preconditioner does not run on.  This is the one place that decides
    whether a 2-D solver reaches the 2-D hierarchy (open/manta_hip_mg2d.h): only with the switch of mantaflow_amd.multigrid2d on.
    The order: a z-slab solver and a backend without the extension first (core._extension_lib; the phrase is the mg2d row's when
    a 2-D solver asks with the switch on, the multigrid row's otherwise), then a 2-D solver with the switch off, then a HIP
    library that was built without the 2-D hierarchy"""
    two_d = _multigrid_2d and not s.is3D()
    if two_d and s.lib.backend == "hip" and tuple(s._slab_window) == (0, 0) and not s.lib.mg2d:
        raise RuntimeError("%s: %s lacks the 2-D multigrid extension (manta_hip_mg2d.h) -- rebuild the library" % (name, s.lib.path))
    lib = _extension_lib(s, name, "mg2d" if two_d else "multigrid")
    if not s.is3D() and not two_d:
        raise RuntimeError("%s: the multigrid preconditioners PcMGStatic / PcMGDynamic run on 3-D solvers only" % name)
    return lib


def _release_mg(solver):
    mg, solver._mg = solver._mg, None
    _mg_solvers.discard(solver)
    if mg is not None:
        mg.release()


@plugin
def releaseMG(solver=None):
    """pressure.cpp:252-267: release the multigrid hierarchy PcMGStatic keeps on a solver (of every solver when none is given)"""
    if solver is None or (isinstance(solver, int) and solver == 0):
        for s in list(_mg_solvers):
            _release_mg(s)
        return
    _release_mg(_chk(solver, core.FluidSolver, "FluidSolver"))


def _fix_pressure(flags, rhs, A0, Ai, Aj, Ak):
    """zero-pressure fixing, pressure.cpp:349-390"""
    s = flags.parent
    ne = ctypes.c_int32(0)
    s.lib.call("mf_count_empty_cells", flags.n, flags.ptr, ctypes.byref(ne), s.stream)
    if ne.value != 0:
        return
    sx, sy, sz = flags.dims
    f = flags.data.view(sz, sy, sx)
    top = (sx // 2, sy - 1, sz // 2 if flags.is3D() else 0)
    fix = -1
    for dy in (0, 1, 2):
        i, j, k = top[0], top[1] - dy, top[2]
        if int(f[k, j, i].item()) & core.TypeFluid:
            fix = i + sx * (j + sy * k)
            break
    if fix == -1:
        inner = f[(slice(1, -1) if flags.is3D() else slice(None)), 1:-1, 1:-1]
        nz = torch.nonzero((inner & core.TypeFluid) != 0)
        if nz.numel():
            k, j, i = (int(v) for v in nz[0])
            k = k + 1 if flags.is3D() else 0
            fix = (i + 1) + sx * ((j + 1) + sy * k)
    if fix >= 0:
        s.lib.call("mf_fix_pressure", sx, sy, sz, int(fix), 0.0, rhs.ptr, A0.ptr, Ai.ptr, Aj.ptr, Ak.ptr, s.stream)


@plugin
def correctVelocity(vel, pressure, flags, cgAccuracy=1e-3, phi=None, perCellCorr=None, fractions=None, gfClamp=1e-04,
                    cgMaxIterFac=1.5, precondition=True, preconditioner=PcMIC, enforceCompatibility=False, useL2Norm=False,
                    zeroPressureFixing=False, curv=None, surfTens=0.):
    _chk(vel, MACGrid, "MACGrid"); _chk(pressure, Grid, "Grid<Real>"); _chk(flags, FlagGrid, "FlagGrid")
    phi, curv = _opt(phi, Grid, "Grid<Real>"), _opt(curv, Grid, "Grid<Real>")
    s = flags.parent
    sx, sy, sz = flags.dims
    s.lib.call("mf_correct_velocity", sx, sy, sz, flags.ptr, vel.ptr, pressure.ptr, s.stream)
    if phi is not None:
        s.lib.call("mf_correct_velocity_ghost_fluid", sx, sy, sz, vel.ptr, flags.ptr, pressure.ptr, phi.ptr, float(gfClamp),
                   None if curv is None else curv.ptr, float(surfTens), s.stream)
        s.lib.call("mf_replace_clamped_ghost_fluid_vels", sx, sy, sz, vel.ptr, flags.ptr, pressure.ptr, phi.ptr, float(gfClamp), s.stream)


@plugin
def solvePressure(vel, pressure, flags, cgAccuracy=1e-3, phi=None, perCellCorr=None, fractions=None, obvel=None, gfClamp=1e-04,
                  cgMaxIterFac=1.5, precondition=True, preconditioner=PcMIC, enforceCompatibility=False, useL2Norm=False,
                  zeroPressureFixing=False, curv=None, surfTens=0., retRhs=None):
    _chk(vel, MACGrid, "MACGrid")
    if precondition is not False and preconditioner in (PcMGDynamic, PcMGStatic):
        _multigrid_lib(vel.parent, "solvePressure")
    if _plain_system(vel, pressure, flags, cgAccuracy, phi, perCellCorr, fractions, obvel, precondition, preconditioner,
                     enforceCompatibility, zeroPressureFixing, curv, surfTens):
        # the plain case (every smoke scene, FLIP without ghost fluid): rhs + packed matrix in one pass, MIC factor and PCG on the
        # packed bytes -- the coefficient grids A0 / Ai / Aj / Ak and pca1..3 of pressure.cpp:332-338, 412-415 are never made
        s = flags.parent
        sx, sy, sz = flags.dims
        rhs, residual, search, tmp, pca0 = (_scratch_grid(s) for _ in range(5))
        maxIter = int(np.float32(cgMaxIterFac) * np.float32(max(sx, sy, sz)))        # pressure.cpp:410 (3D)
        out = (ctypes.c_float * 3)()
        took = True
        try:
            s.lib.call("mf_solve_pressure_fused", sx, sy, sz, flags.ptr, vel.ptr, pressure.ptr, rhs.ptr, residual.ptr, search.ptr, tmp.ptr,
                       pca0.ptr, float(cgAccuracy), int(maxIter), int(bool(useL2Norm)), out, s.stream)
        except RuntimeError as e:
            # the library declines before it touches anything (e.g. mf_set_mic_mode("levels")): the three-call path below
            if not str(e).startswith("mf_solve_pressure_fused: needs"):
                raise
            took = False
        if took:
            _last_cg["iterations"], _last_cg["residual"] = int(out[0]), float(out[1])
            correctVelocity(vel, pressure, flags, notiming=True)
            if retRhs is not None and not (isinstance(retRhs, int) and retRhs == 0):
                _chk(retRhs, Grid, "Grid<Real>").copyFrom(rhs)
            return
        del rhs, residual, search, tmp, pca0
    rhs = Grid(vel.parent)
    common = dict(cgAccuracy=cgAccuracy, phi=phi, perCellCorr=perCellCorr, fractions=fractions, gfClamp=gfClamp,
                  cgMaxIterFac=cgMaxIterFac, precondition=precondition, preconditioner=preconditioner,
                  enforceCompatibility=enforceCompatibility, useL2Norm=useL2Norm, zeroPressureFixing=zeroPressureFixing,
                  curv=curv, surfTens=surfTens, notiming=True)
    computePressureRhs(rhs, vel, pressure, flags, obvel=obvel, **common)
    solvePressureSystem(rhs, vel, pressure, flags, **common)
    correctVelocity(vel, pressure, flags, **common)
    if retRhs is not None and not (isinstance(retRhs, int) and retRhs == 0):
        _chk(retRhs, Grid, "Grid<Real>").copyFrom(rhs)


def _scratch_grid(s, cls=None):
    """a temp grid from the solver's pool WITHOUT the clear of the Grid constructor, for callees that overwrite every cell"""
    cls = cls or Grid
    g = cls.__new__(cls)
    core.PbClass.__init__(g, s, "")
    g.sx, g.sy, g.sz = s.mGridSize
    g.n = g.sx * g.sy * g.sz
    g.data = s._alloc(g._kind, zero=False)
    g._external = False
    return g


def _plain_system(vel, pressure, flags, cgAccuracy, phi, perCellCorr, fractions, obvel, precondition, preconditioner,
                  enforceCompatibility, zeroPressureFixing, curv, surfTens):
    """can mf_solve_pressure_fused take this solvePressure call?  (3D, rows of a multiple of 8 cells, MIC, MakeLaplaceMatrix system
    with the plain MakeRhs)"""
    if not (isinstance(pressure, Grid) and isinstance(flags, FlagGrid)) or not flags.is3D():
        return False
    none = lambda v: v is None or (isinstance(v, int) and not isinstance(v, bool) and v == 0)
    if not (none(phi) and none(perCellCorr) and none(fractions) and none(obvel) and none(curv)):
        return False
    if precondition is not True or preconditioner != PcMIC or enforceCompatibility or zeroPressureFixing or cgAccuracy < 1e-07:
        return False
    if flags.sx % 8 != 0 or _fused_off:
        return False
    return (vel.sx, vel.sy, vel.sz) == flags.dims == (pressure.sx, pressure.sy, pressure.sz)


_fused_off = bool(__import__("os").environ.get("MF_NO_FUSED_SETUP"))


def lastCgStats():
    """iterations / residual of the most recent solvePressureSystem (the reference prints them at debug level 2,
    pressure.cpp:442)"""
    return dict(_last_cg)


# =========================================================================================================
# FLIP transfers
# =========================================================================================================
_deterministic_p2g = True


def setDeterministicP2G(on):
    """particle->grid transfers: True (default) = sums in particle-index order, bit-identical to the reference's
    single-threaded scatter (flip.cpp:619) on every run (parallel ordered gather, p2g_ordered.hip; 2.2 ms for 3.8 M
    particles at 128^3); False = fp32 atomics with block-private LDS accumulation (1.6 ms, last bits depend on the order
    of arrival)"""
    global _deterministic_p2g
    _deterministic_p2g = bool(on)


def _pargs(parts, ptype):
    return (parts.np, parts.cap, _ptr(parts.pos), _ptr(parts.flag)), (None if ptype is None else ptype.ptr)


@plugin
def mapPartsToMAC(flags, vel, velOld, parts, partVel, weight=None, ptype=None, exclude=0):
    _chk(flags, FlagGrid, "FlagGrid"); _chk(vel, MACGrid, "MACGrid"); _chk(velOld, MACGrid, "MACGrid")
    weight = _opt(weight, VecGrid, "Grid<Vec3>")
    s = flags.parent
    w = weight if weight is not None else VecGrid(s)
    (np_, cap, pos, pfl), pt = _pargs(parts, ptype)
    s.lib.call("mf_map_parts_to_mac", flags.sx, flags.sy, flags.sz, vel.ptr, velOld.ptr, w.ptr, np_, cap, pos, pfl,
               partVel.ptr, pt, int(exclude), int(_deterministic_p2g), s.stream)


@plugin
def mapMACToParts(flags, vel, parts, partVel, ptype=None, exclude=0):
    s = flags.parent
    (np_, cap, pos, pfl), pt = _pargs(parts, ptype)
    s.lib.call("mf_map_mac_to_parts", flags.sx, flags.sy, flags.sz, vel.ptr, np_, cap, pos, pfl, partVel.ptr, pt, int(exclude), s.stream)


@plugin
def flipVelocityUpdate(flags, vel, velOld, parts, partVel, flipRatio, ptype=None, exclude=0):
    s = flags.parent
    (np_, cap, pos, pfl), pt = _pargs(parts, ptype)
    s.lib.call("mf_flip_velocity_update", flags.sx, flags.sy, flags.sz, vel.ptr, velOld.ptr, np_, cap, pos, pfl,
               partVel.ptr, float(flipRatio), pt, int(exclude), s.stream)


@plugin
def getComponent(source, target, component):
    """grid.cpp:743-746: target = source[component] (a plane copy in the SoA layout)"""
    _chk(source, VecGrid, "Grid<Vec3>"); _chk(target, Grid, "Grid<Real>")
    s = source.parent
    s.lib.call("mf_copy_f32", target.n, target.ptr, _ptr(source.data[int(component) * source.n:]), s.stream)


@plugin
def setComponent(source, target, component):
    """grid.cpp:748-751: target[component] = source"""
    _chk(source, Grid, "Grid<Real>"); _chk(target, VecGrid, "Grid<Vec3>")
    s = source.parent
    s.lib.call("mf_copy_f32", source.n, _ptr(target.data[int(component) * target.n:]), source.ptr, s.stream)


@plugin
def resetOutflow(flags, phi=None, parts=None, real=None, index=None, indexSys=None):
    """extforces.cpp:134-161 (index / indexSys only speed up the reference's particle loop; same result without)"""
    _chk(flags, FlagGrid, "FlagGrid")
    phi, real = _opt(phi, Grid, "Grid<Real>"), _opt(real, Grid, "Grid<Real>")
    s = flags.parent
    np_, cap, pos, pfl = (0, 0, None, None) if parts is None else _pargs(parts, None)[0]
    s.lib.call("mf_reset_outflow", flags.sx, flags.sy, flags.sz, flags.ptr, None if phi is None else phi.ptr,
               None if real is None else real.ptr, np_, cap, pos, pfl, s.stream)


@plugin
def apicMapPartsToMAC(flags, vel, parts, partVel, cpx, cpy, cpz, mass=None, ptype=None, exclude=0):
    """plugin/apic.cpp:92-110; the scatter is summed in particle-index order per node (= the reference's serial kernel)"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(vel, MACGrid, "MACGrid")
    mass = _opt(mass, MACGrid, "MACGrid")
    s = flags.parent
    m = mass if mass is not None else MACGrid(s)
    (np_, cap, pos, pfl), pt = _pargs(parts, ptype)
    s.lib.call("mf_apic_map_parts_to_mac", flags.sx, flags.sy, flags.sz, vel.ptr, m.ptr, np_, cap, pos, pfl, partVel.ptr,
               cpx.ptr, cpy.ptr, cpz.ptr, pt, int(exclude), s.stream)


@plugin
def apicMapMACGridToParts(partVel, cpx, cpy, cpz, parts, vel, flags, ptype=None, exclude=0):
    """plugin/apic.cpp:175-181"""
    _chk(vel, MACGrid, "MACGrid")
    s = flags.parent
    (np_, cap, pos, pfl), pt = _pargs(parts, ptype)
    s.lib.call("mf_apic_map_mac_to_parts", flags.sx, flags.sy, flags.sz, vel.ptr, np_, cap, pos, pfl, partVel.ptr,
               cpx.ptr, cpy.ptr, cpz.ptr, pt, int(exclude), s.stream)


def _map_parts_to_grid(flags, target, parts, source, ncomp):
    s = flags.parent
    tmp = Grid(s)
    (np_, cap, pos, pfl), _ = _pargs(parts, None)
    s.lib.call("mf_map_parts_to_grid", flags.sx, flags.sy, flags.sz, ncomp, target.ptr, tmp.ptr, np_, cap, pos, pfl,
               source.ptr, int(_deterministic_p2g), s.stream)


@plugin
def mapPartsToGrid(flags, target, parts, source): _map_parts_to_grid(flags, _chk(target, Grid, "Grid<Real>"), parts, source, 1)


@plugin
def mapPartsToGridVec3(flags, target, parts, source): _map_parts_to_grid(flags, _chk(target, VecGrid, "Grid<Vec3>"), parts, source, 3)


@plugin
def mapGridToParts(source, parts, target):
    s = source.parent
    (np_, cap, pos, pfl), _ = _pargs(parts, None)
    s.lib.call("mf_map_grid_to_parts", source.sx, source.sy, source.sz, 1, source.ptr, np_, cap, pos, pfl, target.ptr, s.stream)


@plugin
def mapGridToPartsVec3(source, parts, target):
    s = source.parent
    (np_, cap, pos, pfl), _ = _pargs(parts, None)
    s.lib.call("mf_map_grid_to_parts", source.sx, source.sy, source.sz, 3, source.ptr, np_, cap, pos, pfl, target.ptr, s.stream)


# =========================================================================================================
# FLIP glue
# =========================================================================================================
@plugin
def extrapolateMACSimple(flags, vel, distance=4, phiObs=None, intoObs=False):
    """fastmarch.cpp:337-376"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(vel, MACGrid, "MACGrid")
    s = flags.parent
    if phiObs is not None and not (isinstance(phiObs, int) and phiObs == 0):
        # knUnprojectNormalComp between the component passes and the into-boundary copy (include/open/manta_hip_movingobs.h)
        lib = _extension_lib(s, "extrapolateMACSimple", "movingobs")
        _chk(phiObs, LevelsetGrid, "LevelsetGrid")
        flags._check_same(phiObs)
        tmp, velTmp = core.IntGrid(s), MACGrid(s)
        lib.call("mf_movingobs_extrapolate_mac_simple", flags.sx, flags.sy, flags.sz, flags.ptr, vel.ptr, int(distance), int(bool(intoObs)),
                 phiObs.ptr, tmp.ptr, velTmp.ptr, s.stream)
        return
    tmp, velTmp = core.IntGrid(s), MACGrid(s)
    s.lib.call("mf_extrapolate_mac_simple", flags.sx, flags.sy, flags.sz, flags.ptr, vel.ptr, int(distance), int(bool(intoObs)),
               tmp.ptr, velTmp.ptr, s.stream)


@plugin
def extrapolateMACFromWeight(vel, weight, distance=2):
    """fastmarch.cpp:415-430"""
    _chk(vel, MACGrid, "MACGrid"); _chk(weight, VecGrid, "Grid<Vec3>")
    s = vel.parent
    s.lib.call("mf_extrapolate_mac_from_weight", vel.sx, vel.sy, vel.sz, vel.ptr, weight.ptr, int(distance), s.stream)


@plugin
def markFluidCells(parts, flags, phiObs=None, ptype=None, exclude=0):
    """flip.cpp:166-188"""
    _chk(flags, FlagGrid, "FlagGrid")
    phiObs = _opt(phiObs, Grid, "Grid<Real>")
    s = flags.parent
    ftmp = core.IntGrid(s) if phiObs is not None else None
    (np_, cap, pos, pfl), pt = _pargs(parts, ptype)
    s.lib.call("mf_mark_fluid_cells", flags.sx, flags.sy, flags.sz, flags.ptr, np_, cap, pos, pfl, pt, int(exclude),
               None if phiObs is None else phiObs.ptr, None if ftmp is None else ftmp.ptr, s.stream)


@plugin
def pushOutofObs(parts, flags, phiObs, shift=0., thresh=0., ptype=None, exclude=0):
    """flip.cpp:584-602"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(phiObs, Grid, "Grid<Real>")
    s = flags.parent
    (np_, cap, pos, pfl), pt = _pargs(parts, ptype)
    s.lib.call("mf_push_out_of_obs", flags.sx, flags.sy, flags.sz, np_, cap, pos, pfl, phiObs.ptr, float(shift), float(thresh),
               pt, int(exclude), s.stream)


# =========================================================================================================
# free-surface pieces of scenes/benchmark_dam.py
# =========================================================================================================
@plugin
def gridParticleIndex(parts, indexSys, flags, index, counter=None):
    """flip.cpp:273-320: index = first slot per cell, indexSys = particle indices ordered by (cell, particle)"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(index, core.IntGrid, "Grid<int>")
    s = flags.parent
    cnt = counter if counter is not None else core.IntGrid(s)
    np_ = parts.np
    if indexSys.data.numel() < max(np_, 1):
        indexSys.data = torch.zeros(max(parts.cap, np_, 1), dtype=torch.int32, device=s.device)
    keys = torch.empty(2 * max(np_, 1), dtype=torch.int32, device=s.device)
    vals = torch.empty(2 * max(np_, 1), dtype=torch.int32, device=s.device)
    n_idx = ctypes.c_int64(0)
    s.lib.call("mf_grid_particle_index", flags.sx, flags.sy, flags.sz, np_, parts.cap, _ptr(parts.pos), _ptr(parts.flag),
               _ptr(indexSys.data), index.ptr, cnt.ptr, _ptr(keys), _ptr(vals), ctypes.byref(n_idx), s.stream)
    indexSys.np = int(n_idx.value)


@plugin
def unionParticleLevelset(parts, indexSys, flags, index, phi, radiusFactor=1., ptype=None, exclude=0):
    """flip.cpp:322-363"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(phi, Grid, "LevelsetGrid")
    s = flags.parent
    s.lib.call("mf_union_particle_levelset", flags.sx, flags.sy, flags.sz, parts.np, parts.cap, _ptr(parts.pos),
               _ptr(indexSys.data), int(indexSys.np), index.ptr, phi.ptr, float(radiusFactor),
               None if ptype is None else ptype.ptr, int(exclude), s.stream)


@plugin
def extrapolateLsSimple(phi, distance=4, inside=False, include_walls=False):
    """fastmarch.cpp:472-522"""
    _chk(phi, Grid, "Grid<Real>")
    s = phi.parent
    tmp = core.IntGrid(s)
    s.lib.call("mf_extrapolate_ls_simple", phi.sx, phi.sy, phi.sz, phi.ptr, int(distance), int(bool(inside)),
               int(bool(include_walls)), tmp.ptr, s.stream)


@plugin
def setPartType(parts, ptype, mark, stype, flags, cflag):
    """ptsplugins.cpp:56-65"""
    _chk(flags, FlagGrid, "FlagGrid")
    s = flags.parent
    s.lib.call("mf_set_part_type", flags.sx, flags.sy, flags.sz, flags.ptr, parts.np, parts.cap, _ptr(parts.pos), ptype.ptr,
               int(mark), int(stype), int(cflag), s.stream)


@plugin
def markIsolatedFluidCell(flags, mark):
    """grid.cpp:987-1011"""
    _chk(flags, FlagGrid, "FlagGrid")
    s = flags.parent
    s.lib.call("mf_mark_isolated_fluid_cell", flags.sx, flags.sy, flags.sz, flags.ptr, int(mark), s.stream)


@plugin
def addForcePvel(vel, a, dt, ptype, exclude):
    """ptsplugins.cpp:20-29"""
    a = core._to_vec3(a)
    s = vel.parent
    s.lib.call("mf_add_force_pvel", vel.size(), vel.cap, vel.ptr, float(a.x), float(a.y), float(a.z), float(dt),
               None if ptype is None else ptype.ptr, int(exclude), s.stream)


@plugin
def updateVelocityFromDeltaPos(parts, vel, x_prev, dt, ptype, exclude):
    """ptsplugins.cpp:31-41"""
    s = vel.parent
    s.lib.call("mf_update_velocity_from_delta_pos", parts.np, parts.cap, _ptr(parts.pos), vel.ptr, x_prev.ptr, float(dt),
               None if ptype is None else ptype.ptr, int(exclude), s.stream)


@plugin
def eulerStep(parts, vel, ptype, exclude):
    """ptsplugins.cpp:43-53"""
    s = vel.parent
    s.lib.call("mf_euler_step", parts.np, parts.cap, _ptr(parts.pos), vel.ptr, s.getDt(), None if ptype is None else ptype.ptr,
               int(exclude), s.stream)


# =========================================================================================================
# resampling between grids of different size (plugin/waveletturbulence.cpp:27-78)
# =========================================================================================================
def _size_factor(source, target, scale, offset, size):
    """calcGridSizeFactorMod, waveletturbulence.cpp:27-34 (fp32 Vec3 arithmetic)"""
    f32 = np.float32
    scale, offset = _to_vec3(scale), _to_vec3(offset)
    s1 = tuple(source.parent.globalGridSize())      # whole-domain sizes (a z-slab's grids hold a window of them)
    s2 = list(target.parent.globalGridSize())
    if size is not None:
        size = tuple(int(v) for v in (size if not isinstance(size, vec3) else (size.x, size.y, size.z)))
        for c in range(3):
            if size[c] > 0:
                s2[c] = size[c]
    sf = [f32(f32(f32(s1[c]) / f32(s2[c])) / f32((scale.x, scale.y, scale.z)[c])) for c in range(3)]
    off = [f32(f32(f32(-f32((offset.x, offset.y, offset.z)[c])) * sf[c]) + f32(sf[c] * f32(0.5))) for c in range(3)]
    return [float(v) for v in sf], [float(v) for v in off]


def _interpolate(target, source, scale, offset, size, orderSpace, ncomp):
    if int(orderSpace) not in (1, 2):
        raise RuntimeError("Unknown interpolation order %s" % orderSpace)
    sf, off = _size_factor(source, target, scale, offset, size)
    s = target.parent
    s.lib.call2(source.parent, "mf_interpolate_grid", target.sx, target.sy, target.sz, target.ptr, source.sx, source.sy, source.sz, source.ptr,
               ncomp, sf[0], sf[1], sf[2], off[0], off[1], off[2], int(orderSpace), s.stream)


@plugin
def interpolateGrid(target, source, scale=vec3(1.), offset=vec3(0.), size=None, orderSpace=1):
    _chk(target, Grid, "Grid<Real>"); _chk(source, Grid, "Grid<Real>")
    _interpolate(target, source, scale, offset, size, orderSpace, 1)


@plugin
def interpolateGridVec3(target, source, scale=vec3(1.), offset=vec3(0.), size=None, orderSpace=1):
    _chk(target, VecGrid, "Grid<Vec3>"); _chk(source, VecGrid, "Grid<Vec3>")
    _interpolate(target, source, scale, offset, size, orderSpace, 3)


@plugin
def interpolateMACGrid(target, source, scale=vec3(1.), offset=vec3(0.), size=None, orderSpace=1):
    _chk(target, MACGrid, "MACGrid"); _chk(source, MACGrid, "MACGrid")
    if int(orderSpace) not in (1, 2):
        raise RuntimeError("Unknown interpolation order %s" % orderSpace)
    sf, off = _size_factor(source, target, scale, offset, size)
    s = target.parent
    s.lib.call2(source.parent, "mf_interpolate_mac_grid", target.sx, target.sy, target.sz, target.ptr, source.sx, source.sy, source.sz,
               source.ptr, sf[0], sf[1], sf[2], off[0], off[1], off[2], int(orderSpace), s.stream)


# =========================================================================================================
# wavelet turbulence pieces of scenes/waveletTurbulence.py
# =========================================================================================================
@plugin
def computeEnergy(flags, vel, energy):
    """waveletturbulence.cpp:180-194"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(vel, MACGrid, "MACGrid"); _chk(energy, Grid, "Grid<Real>")
    s = flags.parent
    s.lib.call("mf_compute_energy", flags.sx, flags.sy, flags.sz, flags.ptr, vel.ptr, energy.ptr, s.stream)


@plugin
def computeWaveletCoeffs(input):
    """waveletturbulence.cpp:197-201 -> WaveletNoiseField::computeCoefficients"""
    _chk(input, Grid, "Grid<Real>")
    s = input.parent
    t1, t2 = Grid(s), Grid(s)
    s.lib.call("mf_compute_wavelet_coeffs", input.sx, input.sy, input.sz, input.ptr, t1.ptr, t2.ptr, s.stream)


@plugin
def vorticityConfinement(vel, flags, strength=0., strengthCell=None):
    """extforces.cpp:409-428"""
    _chk(vel, MACGrid, "MACGrid"); _chk(flags, FlagGrid, "FlagGrid")
    strengthCell = _opt(strengthCell, Grid, "Grid<Real>")
    s = flags.parent
    vc, curl, force, nrm = VecGrid(s), VecGrid(s), VecGrid(s), Grid(s)
    s.lib.call("mf_vorticity_confinement", flags.sx, flags.sy, flags.sz, vel.ptr, flags.ptr, float(strength),
               None if strengthCell is None else strengthCell.ptr, vc.ptr, curl.ptr, nrm.ptr, force.ptr, s.stream)


@plugin
def applyNoiseVec3(flags, target, noise, scale=1.0, scaleSpatial=1.0, weight=None, uv=None):
    """waveletturbulence.cpp:120-178 (weight and uv grids of any size: sampled with getInterpolated when it differs from the target's)"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(target, VecGrid, "Grid<Vec3>")
    weight = _opt(weight, Grid, "Grid<Real>")
    uv = _opt(uv, VecGrid, "Grid<Vec3>")
    if uv is not None and weight is not None and uv.dims != weight.dims:
        raise RuntimeError("UV and weight grid have to match!")
    s = flags.parent
    w = (None, 0, 0, 0) if weight is None else (weight.ptr, weight.sx, weight.sy, weight.sz)
    u = (None, 0, 0, 0) if uv is None else (uv.ptr, uv.sx, uv.sy, uv.sz)
    src = uv.parent if uv is not None else (s if weight is None else weight.parent)
    s.lib.call2(src, "mf_apply_noise_vec3", flags.sx, flags.sy, flags.sz, flags.ptr, target.ptr, _ptr(noise._tile), noise._params(),
                float(scale), float(scaleSpatial), w[0], w[1], w[2], w[3], u[0], u[1], u[2], u[3], s.stream)


@plugin
def setOpenBound(flags, bWidth, openBound="", type=16 | 4):
    """extforces.cpp:106-131 (scene set-up: flag edit on the host)"""
    _chk(flags, FlagGrid, "FlagGrid")
    if openBound == "":
        return
    lo = {c: (c in openBound) for c in "xyz"}
    up = {c: (c.upper() in openBound) for c in "xyz"}
    f = flags.to_numpy()
    sz, sy, sx = f.shape
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    bw = int(bWidth)
    loX, loY = lo["x"] & (i <= bw), lo["y"] & (j <= bw)
    upX, upY = up["x"] & (i >= sx - bw - 1), up["y"] & (j >= sy - bw - 1)
    inI, inJ = (i > bw) & (i < sx - bw - 1), (j > bw) & (j < sy - bw - 1)
    obs = (f & core.TypeObstacle) != 0
    if not flags.is3D():
        m = (loX | upX | loY | upY) & (loX | upX | inI) & (loY | upY | inJ) & obs
    else:
        loZ, upZ = lo["z"] & (k <= bw), up["z"] & (k >= sz - bw - 1)
        inK = (k > bw) & (k < sz - bw - 1)
        m = (loX | upX | loY | upY | loZ | upZ) & (loX | upX | inI) & (loY | upY | inJ) & (loZ | upZ | inK) & obs
    f[m] = int(type)
    flags.from_numpy(f)


# =========================================================================================================
# glue
# =========================================================================================================
@plugin
def setWallBcs(flags, vel, obvel=None, fractions=None, phiObs=None, boundaryWidth=0):
    obvel = _opt(obvel, MACGrid, "MACGrid")
    s = flags.parent
    fractions, phiObs = _opt(fractions, MACGrid, "MACGrid"), _opt(phiObs, Grid, "Grid<Real>")
    if fractions is not None and phiObs is not None:
        # KnSetWallBcsFrac + vel.swap(tmpvel), extforces.cpp:240-335 (obvel and boundaryWidth unused there as well); in place
        lib = _extension_lib(s, "setWallBcs", "obstacles")
        scratch = _wall_frac_scratch(s)
        lib.call("mf_set_wall_bcs_frac", flags.sx, flags.sy, flags.sz, flags.ptr, vel.ptr, phiObs.ptr, _ptr(scratch), scratch.numel(),
                 s.stream)
        return
    s.lib.call("mf_set_wall_bcs", flags.sx, flags.sy, flags.sz, flags.ptr, vel.ptr, None if obvel is None else obvel.ptr, s.stream)


# =========================================================================================================
# fill-fraction obstacle boundaries (include/manta_hip_obstacles.h)
# =========================================================================================================
def _wall_frac_scratch(s):
    """per-solver scratch of mf_set_wall_bcs_frac (new face values + one bit per face), allocated once; never initialised"""
    sc = getattr(s, "_wall_frac_scratch", None)
    if sc is None:
        words = ctypes.c_int64(0)
        s.lib.call("mf_set_wall_bcs_frac_scratch_words", s.mGridSize[0], s.mGridSize[1], s.mGridSize[2], ctypes.byref(words))
        sc = torch.empty(int(words.value), dtype=torch.int32, device=s.device)
        s._wall_frac_scratch = sc
    return sc


@plugin
def updateFractions(flags, phiObs, fractions, boundaryWidth=0, fracThreshold=0.01):
    """initplugins.cpp:436-440: fractions.setConst(0) + KnUpdateFractions (the serial-sweep result)"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(phiObs, Grid, "Grid<Real>"); _chk(fractions, MACGrid, "MACGrid")
    s = flags.parent
    lib = _extension_lib(s, "updateFractions", "obstacles")
    lib.call("mf_update_fractions", flags.sx, flags.sy, flags.sz, flags.ptr, phiObs.ptr, fractions.ptr, int(boundaryWidth),
             float(np.float32(fracThreshold)), s.stream)


@plugin
def setObstacleFlags(flags, phiObs, fractions=None, phiOut=None, phiIn=None, boundaryWidth=1):
    """initplugins.cpp:470-474 -> KnUpdateFlagsObs"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(phiObs, Grid, "Grid<Real>")
    fractions = _opt(fractions, MACGrid, "MACGrid")
    phiOut, phiIn = _opt(phiOut, Grid, "Grid<Real>"), _opt(phiIn, Grid, "Grid<Real>")
    s = flags.parent
    lib = _extension_lib(s, "setObstacleFlags", "obstacles")
    lib.call("mf_set_obstacle_flags", flags.sx, flags.sy, flags.sz, flags.ptr, phiObs.ptr, None if fractions is None else fractions.ptr,
             None if phiOut is None else phiOut.ptr, None if phiIn is None else phiIn.ptr, int(boundaryWidth), s.stream)


_INFLOW_SIDES = {"x": 1, "X": 2, "y": 4, "Y": 8, "z": 16, "Z": 32}


@plugin
def setInflowBcs(vel, dir, value):
    """extforces.cpp:171-182 -> KnSetInflow per character; a bad character raises after the characters before it were applied"""
    _chk(vel, MACGrid, "MACGrid")
    v = _to_vec3(value)
    s = vel.parent
    lib = _extension_lib(s, "setInflowBcs", "obstacles")
    sides, bad = 0, False
    for ch in str(dir):
        if ch not in _INFLOW_SIDES:
            bad = True
            break
        sides |= _INFLOW_SIDES[ch]
    lib.call("mf_set_inflow_bcs", vel.sx, vel.sy, vel.sz, vel.ptr, sides, float(_f32(v.x)), float(_f32(v.y)), float(_f32(v.z)), s.stream)
    if bad:
        raise RuntimeError("invalid character in direction string. Only [xyzXYZ] allowed.")


@plugin
def addNoise(flags, density, noise, sdf=None, scale=1.0):
    """initplugins.cpp:45-51 -> KnAddNoise"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(density, Grid, "Grid<Real>")
    sdf = _opt(sdf, Grid, "Grid<Real>")
    s = flags.parent
    lib = _extension_lib(s, "addNoise", "obstacles")
    lib.call("mf_add_noise", flags.sx, flags.sy, flags.sz, flags.ptr, density.ptr, None if sdf is None else sdf.ptr, _ptr(noise._tile),
             noise._params(), float(_f32(scale)), s.stream)


# =========================================================================================================
# particle resampling for narrow-band FLIP (include/manta_hip_resample.h)
# =========================================================================================================
_seed_reals = {}     # device -> the first reals of RandomStream(9832), which every adjustNumber call restarts


def _seed_table(device, n):
    """at least n reals of the MT19937(9832) stream on the device: one table per process, lengthened when a call needs more"""
    t = _seed_reals.get(device)
    if t is None or t.numel() < n:
        from .scene import RandomStream
        m = max(n, 2 * (t.numel() if t is not None else 0), 1 << 16)
        t = torch.from_numpy(RandomStream(9832).reals(m)).to(device)
        _seed_reals[device] = t
    return t


def calculateRadiusFactor(grid, factor):
    """flip.cpp:198-200: the particle radius that covers a cell's diagonal (double arithmetic, narrowed to Real)"""
    return float(np.float32((np.sqrt(3.) if grid.is3D() else np.sqrt(2.)) * (float(np.float32(factor)) + .01)))


adjustNumberStats = {}      # rounds / kills / inserted / compresses of the last adjustNumber call


@plugin
def adjustNumber(parts, vel, flags, minParticles, maxParticles, phi, radiusFactor=1., narrowBand=-1., exclude=None):
    """plugin/flip.cpp:204-262: cull particles outside the liquid, below the band and in crowded cells, seed thin cells, with
    ParticleSystem::kill's bookkeeping (particle.h:423-427: a mid-loop compress where parts.mAllowCompress, which a
    BasicParticleSystem clears, so there the one compress is doCompress at the end) and insertBufferedParticles (particle.h:636-663).  The serial
    particle loop runs as rounds of its order-free statement ("Particle resampling"): one scalar read-back per round
    and one for the number of new particles; no particle or grid array crosses to the host."""
    _chk(parts, core.BasicParticleSystem, "BasicParticleSystem"); _chk(vel, MACGrid, "MACGrid"); _chk(flags, FlagGrid, "FlagGrid")
    _chk(phi, LevelsetGrid, "LevelsetGrid")
    exclude = _opt(exclude, Grid, "Grid<Real>")
    s = vel.parent
    lib = _extension_lib(s, "adjustNumber", "resample")
    minParticles, maxParticles = _coerce(minParticles, 0), _coerce(maxParticles, 0)
    nb = float(np.float32(narrowBand))
    sls = -calculateRadiusFactor(phi, radiusFactor)
    dims = (flags.sx, flags.sy, flags.sz)
    tmp = core.IntGrid(s)          # Grid<int> tmp(vel.getParent()): zeroed
    res = (ctypes.c_int64 * 4)()
    i0, rounds, kills, compresses = 0, 0, 0, 0
    while i0 < parts.np:
        # without mAllowCompress (a BasicParticleSystem as the reference builds it) no kill compresses: one round does the loop
        chunk = parts.mDeleteChunk if parts.mAllowCompress else (1 << 62)
        lib.call("mf_resample_round", *dims, phi.ptr, tmp.ptr, parts.np, parts.cap, _ptr(parts.pos), _ptr(parts.flag), i0,
                 maxParticles, nb, sls, parts.mDeletes, chunk, res, s.stream)
        rounds += 1
        kills += int(res[1])
        if res[0] < 0:
            parts.mDeletes += int(res[1])
            break
        parts.compress(planned=(int(res[2]), int(res[3])))
        compresses += 1
        i0 = int(res[0]) + 1
    if parts.mDeletes > parts.mDeleteChunk:     # doCompress, particle.h:142-145
        parts.compress()
        compresses += 1
    offsets = core.IntGrid(s)
    total = ctypes.c_int64(0)
    lib.call("mf_resample_seed_plan", *dims, flags.ptr, phi.ptr, None if exclude is None else exclude.ptr, tmp.ptr, minParticles, nb, sls,
             parts.np, _ptr(parts.flag), offsets.ptr, ctypes.byref(total), s.stream)
    total = int(total.value)
    if total:
        old = parts.np
        parts.reserve(old + total)
        parts.resizeAll(old + total, parts.cap)
        reals = _seed_table(s.device, 3 * total)
        lib.call("mf_resample_seed_insert", *dims, offsets.ptr, _ptr(reals), old, total, parts.cap, _ptr(parts.pos), _ptr(parts.flag),
                 s.stream)
        for pd in parts.pdata:
            src = pd.mpGridSource
            mode = 0 if src is None else (2 if pd.mGridSourceMAC else 1)
            if src is not None and (src.sx, src.sy, src.sz) != dims:
                raise RuntimeError("adjustNumber: the source grid of a pdata channel has another resolution")
            if pd.cap != parts.cap:
                raise RuntimeError("adjustNumber: a pdata channel does not follow the capacity of its particle system")
            lib.call("mf_pdata_init_new", *dims, None if src is None else src.ptr, mode, pd._ncomp, old, total, pd.cap, _ptr(parts.pos),
                     pd.ptr, s.stream)
    adjustNumberStats.clear()
    adjustNumberStats.update(rounds=rounds, kills=kills, inserted=total, compresses=compresses)


@plugin
def combineGridVel(vel, weight, combineVel, phi=None, narrowBand=0.0, thresh=0.0):
    """plugin/flip.cpp:748-776 -> knCombineVels: where the particles carry a velocity (weight > thresh) and the face is not deeper
    than narrowBand, combineVel takes vel and vel becomes -1; elsewhere vel becomes 0"""
    _chk(vel, MACGrid, "MACGrid"); _chk(weight, VecGrid, "Grid<Vec3>"); _chk(combineVel, MACGrid, "MACGrid")
    phi = _opt(phi, LevelsetGrid, "LevelsetGrid")
    s = vel.parent
    lib = _extension_lib(s, "combineGridVel", "resample")
    lib.call("mf_combine_grid_vel", vel.sx, vel.sy, vel.sz, vel.ptr, weight.ptr, combineVel.ptr, None if phi is None else phi.ptr,
             float(np.float32(narrowBand)), float(np.float32(thresh)), s.stream)


# =========================================================================================================
# implicit density projection: the position solve of IDP-FLIP / IDP-APIC (include/manta_hip_idp.h)
# =========================================================================================================
@plugin
def copyFlagsToFlags(source, target):
    """implicitdensityprojection.cpp:336-341: target = source, cell by cell (every backend)"""
    _chk(source, FlagGrid, "FlagGrid"); _chk(target, FlagGrid, "FlagGrid")
    target.copyFrom(source)


def _mark_fluid_and_boundary(lib, s, particles, flags, deltaX, phiObs, ptype, exclude):
    (np_, cap, pos, pfl), pt = _pargs(particles, ptype)
    res = (ctypes.c_int64 * 2)()
    lib.call("mf_idp_mark", flags.sx, flags.sy, flags.sz, flags.ptr, deltaX.ptr, phiObs.ptr, np_, cap, pos, pfl, pt, int(exclude),
             res, s.stream)
    return int(res[0]), int(res[1])


markFluidAndBoundaryCellsStats = {}      # particles inside obstacle cells / of them pushing out, of the last call


@plugin
def markFluidAndBoundaryCells(particles, flags, deltaX, phiObs, ptype=None, exclude=0):
    """implicitdensityprojection.cpp:29-79: fluid cells become empty, deltaX is cleared, every cell holding an active particle
    (not excluded) becomes fluid, and a particle inside an obstacle cell with phiObs <= 0 proposes the displacement that pushes it
    out on the faces of its cell; a face keeps the proposal of largest magnitude, among equal ones the lowest particle's (the
    serial loop, stated order-free: DESIGN.md, "Implicit density projection").  In 2-D no z component is written.  Cells that
    carry the obstacle bit together with the empty or fluid bit (no flag initialiser makes them) are marked and propose nothing.
    One scalar read-back (two when a particle sits in an obstacle cell); no array crosses to the host."""
    _chk(particles, core.BasicParticleSystem, "BasicParticleSystem"); _chk(flags, FlagGrid, "FlagGrid")
    _chk(deltaX, MACGrid, "MACGrid"); _chk(phiObs, Grid, "Grid<Real>")
    ptype = _opt(ptype, core.PdataInt, "ParticleDataImpl<int>")
    s = flags.parent
    lib = _extension_lib(s, "markFluidAndBoundaryCells", "idp")
    inside, pushing = _mark_fluid_and_boundary(lib, s, particles, flags, deltaX, phiObs, ptype, exclude)
    markFluidAndBoundaryCellsStats.clear()
    markFluidAndBoundaryCellsStats.update(boundary_particles=inside, pushing=pushing)


mapMassToGridStats = {}      # rounds / candidates / flipped cells / boundary particles / read-backs of the last mapMassToGrid call


@plugin
def mapMassToGrid(flags, density, parts, source, deltaX, phiObs, dt, particleMass, noDensityClamping=False):
    """implicitdensityprojection.cpp:156-180: markFluidAndBoundaryCells (no ptype), density = the sum of the particles' trilinear
    weights (the ordered, bit-exact particle->grid transfer; `source` only feeds the transfer's discarded value grid), then
    knComputeDensity: 1 - density * particleMass minus the divergence of the push-out displacements and -- in 3-D -- the particle
    deficiency of obstacle and empty neighbours; surface cells left positive become empty (flag TypeEmpty exactly, density 0);
    the clamp to +-0.5 and the division by dt unless noDensityClamping; 0 in non-fluid cells.  The 3-D kernel of the reference
    reads the flags it rewrites: the contract is its single-thread sweep (k outer, j, i inner), computed in rounds over the cells
    whose flip depends on earlier flips ("Implicit density projection").  Fluid cells on the outermost layer of the
    grid make the reference read out of bounds: the contract covers domains whose outermost layer is not fluid
    (initDomain(boundaryWidth >= 1)); there a neighbour outside the grid counts as neither obstacle nor empty.  Scalar read-backs
    only (mapMassToGridStats counts them); no grid or particle array crosses to the host."""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(density, Grid, "Grid<Real>"); _chk(parts, core.BasicParticleSystem, "BasicParticleSystem")
    _chk(source, core.PdataReal, "ParticleDataImpl<Real>"); _chk(deltaX, MACGrid, "MACGrid"); _chk(phiObs, Grid, "Grid<Real>")
    s = flags.parent
    lib = _extension_lib(s, "mapMassToGrid", "idp")
    inside, pushing = _mark_fluid_and_boundary(lib, s, parts, flags, deltaX, phiObs, None, 0)
    (np_, cap, pos, pfl), _ = _pargs(parts, None)
    dims = (flags.sx, flags.sy, flags.sz)
    if source.cap != parts.cap:
        raise RuntimeError("mapMassToGrid: the source channel does not follow the capacity of its particle system")
    lib.call("mf_idp_map_weights", *dims, density.ptr, np_, cap, pos, pfl, source.ptr, s.stream)
    res = (ctypes.c_int64 * 4)()
    lib.call("mf_idp_compute_density", *dims, density.ptr, flags.ptr, deltaX.ptr, float(np.float32(dt)), float(np.float32(particleMass)),
             int(noDensityClamping), res, s.stream)
    mapMassToGridStats.clear()
    mapMassToGridStats.update(rounds=int(res[2]), candidates=int(res[0]), flipped=int(res[1]), boundary_particles=inside,
                              pushing=pushing, readbacks=2 + (1 if inside else 0))


@plugin
def computeDeltaX(deltaX, Lambda, flags):
    """implicitdensityprojection.cpp:184-205: Lambda = 0 in empty cells (one cell off the sides), then for every non-obstacle cell
    each face component becomes the backward difference of Lambda where the lower neighbour is no obstacle; all other components
    keep their value (the push-out displacements of the marking).  For a non-obstacle cell at i = 0, j = 0 or k = 0 the reference
    reads before the row; here that neighbour counts as an obstacle."""
    _chk(deltaX, MACGrid, "MACGrid"); _chk(Lambda, Grid, "Grid<Real>"); _chk(flags, FlagGrid, "FlagGrid")
    s = flags.parent
    lib = _extension_lib(s, "computeDeltaX", "idp")
    lib.call("mf_idp_compute_delta_x", flags.sx, flags.sy, flags.sz, flags.ptr, deltaX.ptr, Lambda.ptr, s.stream)


@plugin
def mapMACToPartPositions(flags, deltaX, parts, dt, ptype=None, exclude=0, mapQuadratic=False):
    """implicitdensityprojection.cpp:207-245: pos += deltaX.getInterpolated(pos) * dt for the active, not excluded particles, then
    per component the clamp to [1.001, size - 1.001] (z of a 2-D solver: [-10.001, 10.001]); mapQuadratic is accepted and
    ignored, as in the reference"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(deltaX, MACGrid, "MACGrid"); _chk(parts, core.BasicParticleSystem, "BasicParticleSystem")
    ptype = _opt(ptype, core.PdataInt, "ParticleDataImpl<int>")
    s = flags.parent
    lib = _extension_lib(s, "mapMACToPartPositions", "idp")
    (np_, cap, pos, pfl), pt = _pargs(parts, ptype)
    lib.call("mf_idp_map_mac_to_positions", flags.sx, flags.sy, flags.sz, deltaX.ptr, np_, cap, pos, pfl, pt, int(exclude),
             float(np.float32(dt)), s.stream)


# =========================================================================================================
# averaged and improved particle level sets (include/manta_hip_partls.h)
# =========================================================================================================
def _particle_levelset(name, improved, parts, indexSys, flags, index, phi, radiusFactor, smoothen, smoothenNeg, t_low, t_high, ptype, exclude):
    _chk(parts, core.BasicParticleSystem, "BasicParticleSystem"); _chk(indexSys, core.ParticleIndexSystem, "ParticleIndexSystem")
    _chk(flags, FlagGrid, "FlagGrid"); _chk(index, core.IntGrid, "Grid<int>"); _chk(phi, LevelsetGrid, "LevelsetGrid")
    ptype = _opt(ptype, core.PdataInt, "ParticleDataImpl<int>")
    s = flags.parent
    lib = _extension_lib(s, name, "partls")
    if ptype is not None and ptype.cap != parts.cap:
        raise RuntimeError("%s: the ptype channel does not follow the capacity of its particle system" % name)
    # Grid<Vec3> save_pAcc, Grid<Real> save_rAcc, LevelsetGrid tmp: from the solver's pool, every cell is written before it is read
    pacc = _scratch_grid(s, VecGrid) if improved else None
    racc = _scratch_grid(s) if improved else None
    tmp = _scratch_grid(s) if (smoothen > 0 or smoothenNeg > 0) else None
    lib.call("mf_partls_levelset", flags.sx, flags.sy, flags.sz, parts.np, parts.cap, _ptr(parts.pos), _ptr(indexSys.data),
             int(indexSys.np), index.ptr, phi.ptr, float(np.float32(radiusFactor)), smoothen, smoothenNeg, int(improved),
             float(np.float32(t_low)), float(np.float32(t_high)), None if ptype is None else ptype.ptr, int(exclude),
             None if pacc is None else pacc.ptr, None if racc is None else racc.ptr, None if tmp is None else tmp.ptr, s.stream)


@plugin
def averagedParticleLevelset(parts, indexSys, flags, index, phi, radiusFactor=1., smoothen=1, smoothenNeg=1, ptype=None, exclude=0):
    """flip.cpp:365-499 (Zhu & Bridson): per cell the particles of the (2r+1)^3 cells around it are averaged with the weights
    max(0, 1 - |x - p|^2 / (4 radius^2)), summed in the reference's order; phi = |x - pAvg| - rAvg, or radius where the weights sum
    to at most 1e-6; then max(smoothen, smoothenNeg) rounds of knSmoothGrid / knSmoothGridNeg and setBound(0.5, 0).  Bit-identical
    to the reference.  Nothing is read back."""
    _particle_levelset("averagedParticleLevelset", False, parts, indexSys, flags, index, phi, radiusFactor, smoothen, smoothenNeg,
                       0.4, 3.5, ptype, exclude)


@plugin
def improvedParticleLevelset(parts, indexSys, flags, index, phi, radiusFactor=1., smoothen=1, smoothenNeg=1, t_low=0.4, t_high=3.5,
                             ptype=None, exclude=0):
    """flip.cpp:501-581 (Solenthaler et al.): the averaged level set, whose radius term is scaled down where the largest eigenvalue
    of the Jacobian of the averaged positions reaches t_low (correctLevelset), before the smoothing rounds.  Bit-identical to the
    reference up to the rounding of the device's fp64 pow / acos / cos / sin (README, "Averaged and improved particle level
    sets").  Nothing is read back."""
    _particle_levelset("improvedParticleLevelset", True, parts, indexSys, flags, index, phi, radiusFactor, smoothen, smoothenNeg,
                       t_low, t_high, ptype, exclude)


# =========================================================================================================
# secondary particles: spray, foam, bubbles (include/manta_hip_secparts.h)
# =========================================================================================================
class _SecondaryStream(object):
    """the `static RandomStream mRand(9832)` of one sampling kernel (secondaryparticles.cpp:118, 175): one per process and mode,
    never restarted by a call; `cursor` counts the reals drawn so far"""

    def __init__(self):
        self.seek(0)

    def seek(self, cursor):
        from .scene import RandomStream
        self.rs, self.cursor = RandomStream(9832), 0
        while self.cursor < cursor:         # MT19937 has no cheap jump: draw and drop
            self.take(min(cursor - self.cursor, 1 << 20))

    def take(self, n):
        self.cursor += n
        return self.rs.reals(n)


_secondary_streams = {}      # mode -> _SecondaryStream


def _secondary_stream(mode):
    if mode not in _secondary_streams:
        _secondary_streams[mode] = _SecondaryStream()
    return _secondary_streams[mode]


def resetSecondaryParticleStreams():
    """restart the random streams of both sampling modes, as a fresh process of the reference has them (no reference counterpart)"""
    _secondary_streams.clear()


def _set_secondary_stream_cursor(mode, cursor):
    """test hook: the stream of `mode` as it is after `cursor` reals"""
    _secondary_stream(mode).seek(int(cursor))


_FLAG_FLUID, _FLAG_OBSTACLE, _FLAG_INFLOW, _FLAG_OUTFLOW = 1, 2, 8, 16
_PTRACER = 16

flipSampleSecondaryParticlesStats = {}     # spawned / reals / stream cursor after the last flipSampleSecondaryParticles call


@plugin
def flipComputeSecondaryParticlePotentials(potTA, potWC, potKE, neighborRatio, flags, v, normal, phi, radius, tauMinTA, tauMaxTA,
                                           tauMinWC, tauMaxWC, tauMinKE, tauMaxKE, scaleFromManta, itype=_FLAG_FLUID,
                                           jtype=_FLAG_OBSTACLE | _FLAG_OUTFLOW | _FLAG_INFLOW):
    """secondaryparticles.cpp:24-103: the four outputs are cleared, normal = GradientOp(phi) on the interior, and every itype cell at
    least `radius` cells from the sides gets the trapped-air, wave-crest and kinetic-energy potentials and the fluid-neighbour
    ratio of its (2 radius + 1)^3 neighbourhood (jtype cells and the outermost layer do not count).  Bit-identical to the
    reference.  A streaming pass writes the per-cell terms into pool scratch, the gather reads only those; nothing is read back.
    radius < 1 is refused (the reference would read outside the grid)."""
    for g in (potTA, potWC, potKE, neighborRatio):
        _chk(g, Grid, "Grid<Real>")
    _chk(flags, FlagGrid, "FlagGrid"); _chk(v, MACGrid, "MACGrid"); _chk(normal, VecGrid, "Grid<Vec3>"); _chk(phi, Grid, "Grid<Real>")
    s = flags.parent
    lib = _extension_lib(s, "flipComputeSecondaryParticlePotentials", "secparts")
    radius = _coerce(radius, 0)
    if radius < 1:
        raise RuntimeError("flipComputeSecondaryParticlePotentials: radius %d < 1" % radius)
    sv, sn, sc = _scratch_grid(s, VecGrid), _scratch_grid(s, VecGrid), _scratch_grid(s, core.IntGrid)
    f = lambda x: float(np.float32(x))
    lib.call("mf_secparts_potentials", flags.sx, flags.sy, flags.sz, potTA.ptr, potWC.ptr, potKE.ptr, neighborRatio.ptr, flags.ptr, v.ptr,
             normal.ptr, phi.ptr, radius, f(tauMinTA), f(tauMaxTA), f(tauMinWC), f(tauMaxWC), f(tauMinKE), f(tauMaxKE), f(scaleFromManta),
             int(itype), int(jtype), sv.ptr, sn.ptr, sc.ptr, 3, s.stream)


def _secondary_dt(s, dt):
    """float timestep = dt; if (dt <= 0) timestep = parent->getDt()"""
    return float(np.float32(dt)) if dt > 0 else float(np.float32(s.getDt()))


def _follows(parts, name, **channels):
    for what, pd in channels.items():
        if pd.sys is not parts or pd.cap != parts.cap:
            raise RuntimeError("%s: %s is not a channel of the particle system" % (name, what))


@plugin
def flipSampleSecondaryParticles(mode, flags, v, pts_sec, v_sec, l_sec, lMin, lMax, potTA, potWC, potKE, neighborRatio, c_s, c_b, k_ta,
                                 k_wc, dt=0., itype=_FLAG_FLUID):
    """secondaryparticles.cpp:105-220: every itype cell ("single") or each of its 8 sub-cylinders ("multiple") spawns
    int(KE * (k_ta * TA + k_wc * WC) * dt) particles in a cylinder along the local velocity, typed by the cell's neighbour ratio.
    The reference's serial loop over all cells with one process-wide random stream per mode is restated order-free: a count
    kernel, a scan that gives every entry its particle and stream offset, one read-back of the two totals, the host draws that
    window of the stream (which continues from call to call; resetSecondaryParticleStreams restarts it), and an emit kernel with
    one thread per new particle.  Counts, order, flags, lifetimes and stream consumption are bit-identical; positions and
    velocities are within 4 r 2^-23 + 3 ulp (cos / sin of the azimuth: README, "Secondary particles").  Every other pdata channel
    of pts_sec gets a zero entry."""
    if mode not in ("single", "multiple"):
        raise ValueError("Unknown mode: use \"single\" or \"multiple\" instead!")
    _chk(flags, FlagGrid, "FlagGrid"); _chk(v, MACGrid, "MACGrid"); _chk(pts_sec, core.BasicParticleSystem, "BasicParticleSystem")
    _chk(v_sec, core.PdataVec3, "ParticleDataImpl<Vec3>"); _chk(l_sec, core.PdataReal, "ParticleDataImpl<Real>")
    for g in (potTA, potWC, potKE, neighborRatio):
        _chk(g, Grid, "Grid<Real>")
    s = flags.parent
    lib = _extension_lib(s, "flipSampleSecondaryParticles", "secparts")
    _follows(pts_sec, "flipSampleSecondaryParticles", v_sec=v_sec, l_sec=l_sec)
    multiple = int(mode == "multiple")
    f = lambda x: float(np.float32(x))
    step = _secondary_dt(s, dt)
    dims = (flags.sx, flags.sy, flags.sz)
    entries = flags.n * (8 if multiple else 1)
    nbytes = ctypes.c_int64(0)
    lib.call("mf_secparts_scan_bytes", entries, ctypes.byref(nbytes))
    dev = s.device
    nraw = torch.empty(entries, dtype=torch.int32, device=dev)
    poff = torch.empty(entries, dtype=torch.int64, device=dev)
    roff = torch.empty(entries, dtype=torch.int64, device=dev)
    tmp = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    totals = (ctypes.c_int64 * 2)()
    lib.call("mf_secparts_sample_plan", *dims, multiple, flags.ptr, potTA.ptr, potWC.ptr, potKE.ptr, f(k_ta), f(k_wc), step, int(itype),
             _ptr(nraw), _ptr(poff), _ptr(roff), _ptr(tmp), int(nbytes.value), totals, s.stream)
    total, nreals = int(totals[0]), int(totals[1])
    stream = _secondary_stream(mode)
    reals = stream.take(nreals)
    if total:
        old = pts_sec.np
        pts_sec.reserve(old + total)
        pts_sec.resizeAll(old + total, pts_sec.cap)
        for pd in pts_sec.pdata:          # add() -> addEntry(): a default entry in every channel, no setSource initialisation
            for c in range(pd._ncomp):
                pd.data[c * pd.cap + old:c * pd.cap + old + total] = 0
        rdev = torch.from_numpy(reals).to(dev)
        lib.call("mf_secparts_sample_emit", *dims, multiple, v.ptr, potTA.ptr, potWC.ptr, potKE.ptr, neighborRatio.ptr, _ptr(nraw),
                 _ptr(poff), _ptr(roff), _ptr(rdev), nreals, old, total, pts_sec.cap, _ptr(pts_sec.pos), _ptr(pts_sec.flag), v_sec.ptr,
                 l_sec.ptr, f(lMin), f(lMax), f(c_s), f(c_b), step, s.stream)
        pts_sec.mDeleteChunk = pts_sec.np // 20      # ParticleSystem::add, particle.h:414-420
    flipSampleSecondaryParticlesStats.clear()
    flipSampleSecondaryParticlesStats.update(spawned=total, reals=nreals, cursor=stream.cursor)


@plugin
def flipUpdateSecondaryParticles(mode, pts_sec, v_sec, l_sec, f_sec, flags, v, neighborRatio, radius, gravity, k_b, k_d, c_s, c_b, dt=0.,
                                 scale=True, exclude=_PTRACER, antitunneling=0, itype=_FLAG_FLUID):
    """secondaryparticles.cpp:225-447: the active, not excluded particles are typed by the neighbour ratio of their cell and advanced:
    spray ballistically, bubbles by buoyancy and drag towards the fluid velocity, foam with the fluid velocity -- "linear": the
    interpolated MAC velocity, "cubic": a cubic-spline average of the centred velocities of the itype cells within `radius`.
    Particles outside the grid, tunnelling into an obstacle at one of the `antitunneling` - 1 samples of their path, or out of
    lifetime are killed; the call ends with doCompress().  Bit-identical to the reference in every slot of every channel.  One
    scalar (the kill count) is read back."""
    if mode not in ("linear", "cubic"):
        raise ValueError("Unknown mode: use \"linear\" or \"cubic\" instead!")
    _chk(pts_sec, core.BasicParticleSystem, "BasicParticleSystem"); _chk(v_sec, core.PdataVec3, "ParticleDataImpl<Vec3>")
    _chk(l_sec, core.PdataReal, "ParticleDataImpl<Real>"); _chk(f_sec, core.PdataVec3, "ParticleDataImpl<Vec3>")
    _chk(flags, FlagGrid, "FlagGrid"); _chk(v, MACGrid, "MACGrid"); _chk(neighborRatio, Grid, "Grid<Real>")
    s = flags.parent
    lib = _extension_lib(s, "flipUpdateSecondaryParticles", "secparts")
    _follows(pts_sec, "flipUpdateSecondaryParticles", v_sec=v_sec, l_sec=l_sec, f_sec=f_sec)
    radius = _coerce(radius, 0)
    f = lambda x: float(np.float32(x))
    g = _to_vec3(gravity)
    gscale = np.float32(s.getDx()) if scale else np.float32(1)      # float gridScale = scale ? getDx() : 1
    gx, gy, gz = (float(np.float32(c) / gscale) for c in (g.x, g.y, g.z))
    kills = ctypes.c_int64(0)
    lib.call("mf_secparts_update", flags.sx, flags.sy, flags.sz, int(mode == "cubic"), pts_sec.np, pts_sec.cap, _ptr(pts_sec.pos),
             _ptr(pts_sec.flag), v_sec.ptr, l_sec.ptr, f_sec.ptr, flags.ptr, v.ptr, neighborRatio.ptr, radius, gx, gy, gz, f(k_b), f(k_d),
             f(c_s), f(c_b), _secondary_dt(s, dt), int(exclude), int(antitunneling), int(itype), ctypes.byref(kills), s.stream)
    pts_sec.mDeletes += int(kills.value)
    pts_sec.doCompress()


@plugin
def flipDeleteParticlesInObstacle(pts, flags):
    """secondaryparticles.cpp:450-476: active particles outside the grid or inside an obstacle or outflow cell are killed, then
    doCompress().  Bit-identical; one scalar (the kill count) is read back."""
    _chk(pts, core.BasicParticleSystem, "BasicParticleSystem"); _chk(flags, FlagGrid, "FlagGrid")
    s = flags.parent
    lib = _extension_lib(s, "flipDeleteParticlesInObstacle", "secparts")
    kills = ctypes.c_int64(0)
    lib.call("mf_secparts_delete_in_obstacle", flags.sx, flags.sy, flags.sz, pts.np, pts.cap, _ptr(pts.pos), _ptr(pts.flag), flags.ptr,
             ctypes.byref(kills), s.stream)
    pts.mDeletes += int(kills.value)
    pts.doCompress()


@plugin
def setFlagsFromLevelset(flags, phi, exclude=_FLAG_OBSTACLE, itype=_FLAG_FLUID):
    """secondaryparticles.cpp:512-522: a cell with phi < 0 and no `exclude` bit becomes itype (the whole flag word)"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(phi, Grid, "Grid<Real>")
    s = flags.parent
    lib = _extension_lib(s, "setFlagsFromLevelset", "secparts")
    lib.call("mf_secparts_flags_from_levelset", flags.n, flags.ptr, phi.ptr, int(exclude), int(itype), s.stream)


@plugin
def setMACFromLevelset(v, phi, c):
    """secondaryparticles.cpp:524-533: v = c in every cell where phi, interpolated at the cell's corner Vec3(i, j, k), is positive"""
    _chk(v, MACGrid, "MACGrid"); _chk(phi, Grid, "Grid<Real>")
    c = _to_vec3(c)
    s = v.parent
    lib = _extension_lib(s, "setMACFromLevelset", "secparts")
    lib.call("mf_secparts_mac_from_levelset", v.sx, v.sy, v.sz, v.ptr, phi.ptr, float(np.float32(c.x)), float(np.float32(c.y)),
             float(np.float32(c.z)), s.stream)


def _f32(x): return np.float32(x)


@plugin
def addBuoyancy(flags, density, vel, gravity, coefficient=1., scale=True):
    g = _to_vec3(gravity)
    s = flags.parent
    gridScale = _f32(flags.getDx()) if scale else _f32(1)     # float gridScale = scale ? flags.getDx() : 1
    dt = _f32(s.getDt())
    f = [_f32(_f32(_f32(-_f32(c)) * dt) / gridScale) * _f32(coefficient) for c in (g.x, g.y, g.z)]   # -gravity*dt/gridScale*coefficient
    s.lib.call("mf_add_buoyancy", flags.sx, flags.sy, flags.sz, flags.ptr, density.ptr, vel.ptr, float(f[0]), float(f[1]), float(f[2]), s.stream)


@plugin
def addGravity(flags, vel, gravity, exclude=None, scale=True):
    g = _to_vec3(gravity)
    s = flags.parent
    gridScale = _f32(flags.getDx()) if scale else _f32(1)
    dt = _f32(s.getDt())
    f = [_f32(_f32(_f32(c) * dt) / gridScale) for c in (g.x, g.y, g.z)]
    exclude = _opt(exclude, Grid, "Grid<Real>")
    s.lib.call("mf_apply_force", flags.sx, flags.sy, flags.sz, flags.ptr, vel.ptr, float(f[0]), float(f[1]), float(f[2]),
               None if exclude is None else exclude.ptr, 1, s.stream)


@plugin
def addGravityNoScale(flags, vel, gravity, exclude=None): addGravity(flags, vel, gravity, exclude, False, notiming=True)


# =========================================================================================================
# primal-dual fluid guiding (include/manta_hip_guiding.h), source/plugin/fluidguiding.cpp
# =========================================================================================================
_blur_precomp = {"radius": -1, "weights": None, "dev": {}}    # gBlurPrecomputed / gBlurKernelRadius / gBlurKernel, :23-25
_last_guiding = {}


def _blur_weights(lib, s, blurRadius):
    """ADMM_precompute_Separable, :217-226: one blur kernel for the whole process; the weights come from the library's host code
    and are uploaded once per device"""
    if _blur_precomp["radius"] < 0:
        if blurRadius < 0:
            raise RuntimeError("PD_fluid_guiding: invalid blur radius %d" % blurRadius)
        w = np.zeros(2 * blurRadius + 1, np.float32)
        lib.call("mf_guiding_weights", int(blurRadius), w.ctypes.data_as(ctypes.c_void_p))
        _blur_precomp.update(radius=int(blurRadius), weights=w, dev={})
    key = str(s.device)
    if key not in _blur_precomp["dev"]:
        _blur_precomp["dev"][key] = torch.from_numpy(_blur_precomp["weights"]).to(s.device)
    return _blur_precomp["dev"][key]


def _guiding_blur2(lib, s, flags, grid, s1, s2, w_dev):
    """applySeparableGaussianBlur twice (:233-234, :246-247)"""
    lib.call("mf_guiding_blur", flags.sx, flags.sy, flags.sz, flags.ptr, grid.ptr, s1.ptr, None if s2 is None else s2.ptr, _ptr(w_dev),
             _blur_precomp["radius"], 2, s.stream)


@plugin
def PD_fluid_guiding(vel, velT, pressure, flags, weight, blurRadius=5, theta=1.0, tau=1.0, sigma=1.0, epsRel=1e-3, epsAbs=1e-3,
                     maxIters=200, phi=None, perCellCorr=None, fractions=None, obvel=None, gfClamp=1e-04, cgMaxIterFac=1.5,
                     cgAccuracy=1e-3, preconditioner=1, zeroPressureFixing=False, curv=None, surfTens=0.):
    """fluidguiding.cpp:294-353 (Inglis et al., "Primal-Dual Optimization for Fluids"): up to maxIters primal-dual iterations, each
    an x update (two separable Gaussian blurs between two fused element-wise kernels), the package's own solvePressure on the
    slack grid z, and a y update whose kernel also yields the two maxima of the stop test -- the one read-back of an iteration.
    Bit-identical to the reference as far as the inner solve is.  lastGuidingStats() has the iteration counts."""
    _chk(vel, MACGrid, "MACGrid"); _chk(velT, MACGrid, "MACGrid"); _chk(pressure, Grid, "Grid<Real>")
    _chk(flags, FlagGrid, "FlagGrid"); _chk(weight, Grid, "Grid<Real>")
    s = vel.parent
    if _blur_precomp["radius"] >= 0 and _blur_precomp["radius"] != blurRadius:
        raise RuntimeError("More than a single blur radius not supported at the moment.")
    lib = _extension_lib(s, "PD_fluid_guiding", "guiding")
    if preconditioner in (PcMGDynamic, PcMGStatic):
        _multigrid_lib(s, "PD_fluid_guiding")               # the inner solve would refuse, but only after the set-up
    for g in (velT, pressure, flags, weight):
        vel._check_same(g)
    w_dev = _blur_weights(lib, s, blurRadius)
    n, is3d = vel.n, s.is3D()
    sig, ta, th = _f32(sigma), _f32(tau), _f32(theta)
    inv_sigma = _f32(1.0 / float(sig))                      # x.multConst(1.0 / sigma): a double quotient, rounded by Vec3(double)
    # velC, Q, invA and the per-iteration temporaries: from the solver's pool, every cell is written before it is read
    velC, Q, xv, vn, s1 = (_scratch_grid(s, MACGrid) for _ in range(5))
    s2 = _scratch_grid(s, MACGrid) if flags.sz > 1 else None
    invA = _scratch_grid(s)
    x, y, z, zn = MACGrid(s), MACGrid(s), MACGrid(s), _scratch_grid(s, MACGrid)
    velC.copyFrom(vel)
    # precomputeQ, :243-250
    Q.copyFrom(velT)
    Q.sub(velC)
    _guiding_blur2(lib, s, flags, Q, s1, s2, w_dev)
    Q.multConst(vec3(2.0))
    Q.addScaled(velC, vec3(float(-sig)))
    lib.call("mf_guiding_inv_a", n, weight.ptr, float(sig), invA.ptr, s.stream)
    cg_its = []
    it = 0
    out = (ctypes.c_float * 2)()
    for it in range(maxIters):
        lib.call("mf_guiding_pre", n, x.ptr, y.ptr, Q.ptr, invA.ptr, xv.ptr, vn.ptr, float(inv_sigma), float(sig), s.stream)
        _guiding_blur2(lib, s, flags, vn, s1, s2, w_dev)
        lib.call("mf_guiding_mid", n, x.ptr, y.ptr, xv.ptr, vn.ptr, invA.ptr, velC.ptr, z.ptr, zn.ptr, float(sig), float(ta), s.stream)
        z, zn = zn, z                                       # zn now holds z0
        solvePressure(z, pressure, flags, cgAccuracy, phi, perCellCorr, fractions, obvel, gfClamp, cgMaxIterFac, True, preconditioner,
                      False, False, zeroPressureFixing, curv, surfTens, notiming=True)
        cg_its.append(_last_cg.get("iterations"))
        lib.call("mf_guiding_post", n, z.ptr, zn.ptr, y.ptr, float(th), out, s.stream)
        rnorm, zmax = _f32(out[0]), _f32(out[1])
        # getEpsDual, :165-168: sqrt(3.0 or 2.0) * eps_abs in double, eps_rel * getMaxAbs() a Real product, the sum rounded to Real
        epsDual = _f32(np.sqrt(3.0 if is3d else 2.0) * float(_f32(epsAbs)) + float(_f32(epsRel) * zmax))
        if (it > 0 and rnorm < epsDual) or it == maxIters - 1:
            break
    vel.copyFrom(z)
    _last_guiding.clear()
    _last_guiding.update(iterations=int(it), cg_iterations=cg_its, rnorm=float(out[0]), epsDual=float(epsDual) if cg_its else 0.0)


@plugin
def releaseBlurPrecomp():
    """fluidguiding.cpp:356-360"""
    _blur_precomp.update(radius=-1, weights=None, dev={})


def lastGuidingStats():
    """of the most recent PD_fluid_guiding: `iterations`, the value the reference prints at :352 (the index of the last primal-dual
    iteration), and `cg_iterations`, the CG iteration count of each inner solve"""
    d = dict(_last_guiding)
    d["cg_iterations"] = list(d.get("cg_iterations", []))
    return d


@plugin
def getSpiralVelocity(flags, vel, strength=1.0, with3D=False):
    """fluidguiding.cpp:171-191: set-up code, on the host (every backend)"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(vel, MACGrid, "MACGrid")
    nx, ny, nz = flags.sx, flags.sy, (flags.sz if with3D else 1)
    midX, midY = _f32(0.5 * float(_f32(nx - 1))), _f32(0.5 * float(_f32(ny - 1)))
    diffX = (midX - np.arange(nx, dtype=np.float32))[None, :]
    diffY = (midY - np.arange(ny, dtype=np.float32))[:, None]
    hyp = np.sqrt(diffX * diffX + diffY * diffY)
    ok = hyp > 0
    safe = np.where(ok, hyp, _f32(1))
    v = vel.to_numpy()
    v[:nz, :, :, 0] = np.where(ok, diffY / safe, v[:nz, :, :, 0])
    v[:nz, :, :, 1] = np.where(ok, -diffX / safe, v[:nz, :, :, 1])
    vel.from_numpy(v)
    vel.multConst(vec3(float(_f32(strength))))


@plugin
def setGradientYWeight(W, minY, maxY, valAtMin, valAtMax):
    """fluidguiding.cpp:194-205: set-up code, on the host (every backend)"""
    _chk(W, Grid, "Grid<Real>")
    minY, maxY = _coerce(minY, 0), _coerce(maxY, 0)
    vmin, vmax = _f32(valAtMin), _f32(valAtMax)
    a = W.to_numpy()
    for j in range(max(minY, 0), min(maxY, W.sy - 1) + 1):
        val = vmin
        if vmax != vmin:
            with np.errstate(all="ignore"):
                ratio = _f32(j - minY) / _f32(maxY - minY)
                val = _f32(float(ratio * vmax) + (1.0 - float(ratio)) * float(vmin))   # Real product + double product
        a[:, j, :] = val
    W.from_numpy(a)


# =========================================================================================================
# the k-epsilon turbulence model, source/plugin/kepsilon.cpp, and the diagnostics of plugin/waveletturbulence.cpp that share its
# stencil (include/ext/manta_hip_turbulence.h; whole-domain solvers only).  Bit-identical; DESIGN.md section 14.
# =========================================================================================================
@plugin
def KEpsilonComputeProduction(vel, k, eps, prod, nuT, strain=None, pscale=1.0):
    """kepsilon.cpp:86-99 in one kernel: KnTurbulenceClamp on every cell (k and eps rewritten), prod / nuT / strain on the interior
    from the clamped values with the centred velocity formed on the fly.  The reference reads the planes k +- 1 unconditionally, so
    a 2-D solver is refused (first: that refusal holds on every backend)."""
    _chk(vel, MACGrid, "MACGrid")
    for g in (k, eps, prod, nuT):
        _chk(g, Grid, "Grid<Real>")
    strain = _opt(strain, Grid, "Grid<Real>")
    s = k.parent
    if not s.is3D():
        raise RuntimeError("KEpsilonComputeProduction: 3-D solvers only")
    lib = _extension_lib(s, "KEpsilonComputeProduction", "turbulence")
    lib.call("mf_turbulence_production", k.sx, k.sy, k.sz, vel.ptr, k.ptr, eps.ptr, prod.ptr, nuT.ptr, None if strain is None else strain.ptr,
             float(pscale), s.stream)


@plugin
def KEpsilonSources(k, eps, prod):
    """kepsilon.cpp:102-126: the source terms over one solver step, both pre-clamps and KnTurbulenceClamp, one kernel"""
    for g in (k, eps, prod):
        _chk(g, Grid, "Grid<Real>")
    s = k.parent
    lib = _extension_lib(s, "KEpsilonSources", "turbulence")
    lib.call("mf_turbulence_sources", k.n, k.ptr, eps.ptr, prod.ptr, s.getDt(), s.stream)


@plugin
def KEpsilonBcs(flags, k, eps, intensity, nu, fillArea):
    """kepsilon.cpp:129-140: k = 1.5 intensity^2 and eps = Cmu k^2 / nu in every cell (fillArea) or in the obstacle cells"""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(k, Grid, "Grid<Real>"); _chk(eps, Grid, "Grid<Real>")
    if not isinstance(fillArea, bool):
        raise RuntimeError("argument is not a boolean")
    s = k.parent
    lib = _extension_lib(s, "KEpsilonBcs", "turbulence")
    lib.call("mf_turbulence_bcs", k.n, flags.ptr, k.ptr, eps.ptr, float(intensity), float(nu), int(fillArea), s.stream)


@plugin
def KEpsilonGradientDiffusion(k, eps, nuT, sigmaU=4.0, vel=None):
    """kepsilon.cpp:143-179: f += LaplaceOp(f) * nuT * (dt / sigma) for k (sigma 1), eps (sigma 1.3) and, where given, the three
    components of vel (sigmaU): three launches.  The stencil reads neighbours of the field it updates, so each launch writes a
    scratch grid of the solver's pool and the two grids swap their storage."""
    for g in (k, eps, nuT):
        _chk(g, Grid, "Grid<Real>")
    vel = _opt(vel, MACGrid, "MACGrid")
    s = k.parent
    lib = _extension_lib(s, "KEpsilonGradientDiffusion", "turbulence")
    dt = _f32(s.getDt())
    coef = (ctypes.c_float * 5)(*[float(dt / _f32(sg)) for sg in (1.0, 1.3, sigmaU, sigmaU, sigmaU)])   # Real dt / Real sigma
    tmp = _scratch_grid(s)
    for npass, f in enumerate((k, eps)):
        lib.call("mf_turbulence_grad_diff", f.sx, f.sy, f.sz, 1, f.ptr, tmp.ptr, nuT.ptr, npass, coef, s.stream)
        f.swap(tmp)
    if vel is not None:
        tmp3 = _scratch_grid(s, VecGrid)
        lib.call("mf_turbulence_grad_diff", vel.sx, vel.sy, vel.sz, 3, vel.ptr, tmp3.ptr, nuT.ptr, 2, coef, s.stream)
        vel.swap(tmp3)


@plugin
def computeStrainRateMag(vel, mag):
    """waveletturbulence.cpp:212-236: mag = S^2 on the interior; the centred velocity of a border cell is 0"""
    _chk(vel, MACGrid, "MACGrid"); _chk(mag, Grid, "Grid<Real>")
    s = vel.parent
    lib = _extension_lib(s, "computeStrainRateMag", "turbulence")
    lib.call("mf_turbulence_strain_mag", vel.sx, vel.sy, vel.sz, vel.ptr, mag.ptr, s.stream)


@plugin
def computeVorticity(vel, vorticity, norm=None):
    """waveletturbulence.cpp:204-209: the curl of the centred velocity on the interior (the border of `vorticity` keeps its values)
    and, where given, its norm in every cell"""
    _chk(vel, MACGrid, "MACGrid"); _chk(vorticity, VecGrid, "Grid<Vec3>")
    norm = _opt(norm, Grid, "Grid<Real>")
    s = vel.parent
    lib = _extension_lib(s, "computeVorticity", "turbulence")
    lib.call("mf_turbulence_vorticity", vel.sx, vel.sy, vel.sz, vel.ptr, vorticity.ptr, None if norm is None else norm.ptr, s.stream)


@plugin
def getCurl(vel, vort, comp):
    """waveletturbulence.cpp:310-316: one component of the curl of the centred velocity, 0 in the border cells"""
    _chk(vel, MACGrid, "MACGrid"); _chk(vort, Grid, "Grid<Real>")
    comp = _coerce(comp, 0)
    s = vel.parent
    lib = _extension_lib(s, "getCurl", "turbulence")
    lib.call("mf_turbulence_curl_component", vel.sx, vel.sy, vel.sz, vel.ptr, vort.ptr, comp, s.stream)


# =========================================================================================================
# fire (source/plugin/fire.cpp), the wave equation (source/plugin/waves.cpp), uv grids (source/grid.cpp:573-627) and
# extrapolateSimpleFlags (source/plugin/waveletturbulence.cpp:239-307): include/open/manta_hip_fields.h, whole-domain solvers only;
# initVortexVelocity (source/plugin/initplugins.cpp:478-503) is host code of the same extension.  DESIGN.md section 15.
# =========================================================================================================
@plugin
def processBurn(fuel, density, react, red=None, green=None, blue=None, heat=None, burningRate=0.75, flameSmoke=1.0, ignitionTemp=1.25,
                maxTemp=1.75, flameSmokeColor=vec3(0.7, 0.7, 0.7)):
    """fire.cpp:22-75, one kernel on the interior: fuel burns down by burningRate * dt, react follows it, the burnt fuel emits smoke
    into density (which is NOT clamped: the reference drops clamp()'s result), heat takes the flame temperature profile and the
    colours mix; red / green / blue / heat are each optional"""
    for g in (fuel, density, react):
        _chk(g, Grid, "Grid<Real>")
    red, green, blue, heat = (_opt(g, Grid, "Grid<Real>") for g in (red, green, blue, heat))
    c = _to_vec3(flameSmokeColor)
    s = fuel.parent
    lib = _extension_lib(s, "processBurn", "fields")
    p = lambda g: None if g is None else g.ptr
    lib.call("mf_fields_process_burn", fuel.sx, fuel.sy, fuel.sz, fuel.ptr, density.ptr, react.ptr, p(red), p(green), p(blue), p(heat),
             float(burningRate), float(flameSmoke), float(ignitionTemp), float(maxTemp), s.getDt(), float(c.x), float(c.y), float(c.z), s.stream)


@plugin
def updateFlame(react, flame):
    """fire.cpp:78-90: flame = sqrt(react) where react > 0, else 0, on the interior"""
    _chk(react, Grid, "Grid<Real>"); _chk(flame, Grid, "Grid<Real>")
    s = react.parent
    lib = _extension_lib(s, "updateFlame", "fields")
    lib.call("mf_fields_update_flame", react.sx, react.sy, react.sz, react.ptr, flame.ptr, s.stream)


@plugin
def calcSecDeriv2d(v, curv):
    """waves.cpp:32-41: the 2-D five-point second derivative on the interior (of every plane of a 3-D grid)"""
    _chk(v, Grid, "Grid<Real>"); _chk(curv, Grid, "Grid<Real>")
    s = v.parent
    lib = _extension_lib(s, "calcSecDeriv2d", "fields")
    lib.call("mf_fields_sec_deriv_2d", v.sx, v.sy, v.sz, v.ptr, curv.ptr, s.stream)


@plugin
def totalSum(height):
    """waves.cpp:46-53: the fp64 sum of the interior, returned as a Real (one scalar read-back)"""
    _chk(height, Grid, "Grid<Real>")
    s = height.parent
    lib = _extension_lib(s, "totalSum", "fields")
    out = ctypes.c_float(0.0)
    lib.call("mf_fields_total_sum", height.sx, height.sy, height.sz, height.ptr, ctypes.byref(out), s.stream)
    return float(out.value)


@plugin
def normalizeSumTo(height, target):
    """waves.cpp:56-60: height *= Real(target / sum of the interior) in every cell; the factor is formed on the device, nothing is
    read back"""
    _chk(height, Grid, "Grid<Real>")
    s = height.parent
    lib = _extension_lib(s, "normalizeSumTo", "fields")
    lib.call("mf_fields_normalize_sum", height.sx, height.sy, height.sz, height.ptr, float(target), s.stream)


@plugin
def cgSolveWE(flags, ut, utm1, out, crankNic=False, cSqr=0.25, cgMaxIterFac=1.5, cgAccuracy=1e-5):
    """waves.cpp:87-147: one implicit step of the wave equation, (I + s L) out = 2 ut - utm1 (+ s L ut with crankNic),
    s = dt^2 cSqr / 2, by the unpreconditioned GridCg<ApplyMatrix/2D> with the L2 norm; then utm1 <-> ut and ut = out.
    lastCgStats() reports the solve."""
    _chk(flags, FlagGrid, "FlagGrid")
    for g in (ut, utm1, out):
        _chk(g, Grid, "Grid<Real>")
    s = flags.parent
    lib = _extension_lib(s, "cgSolveWE", "fields")
    st = s.stream
    sx, sy, sz = flags.dims
    residual, search, tmp = (Grid(s) for _ in range(3))
    rhs = _scratch_grid(s)                      # written in every cell by the set-up kernel
    A0, Ai, Aj, Ak = (Grid(s) for _ in range(4))
    out.clear()
    lib.call("mf_make_laplace_matrix", sx, sy, sz, flags.ptr, A0.ptr, Ai.ptr, Aj.ptr, Ak.ptr, None, st)
    dt = _f32(s.getDt())
    sc = _f32(float(dt * dt * _f32(cSqr)) * 0.5)            # Real s = dt*dt*cSqr * 0.5: an fp32 product, halved in double
    lib.call("mf_fields_wave_system", sx, sy, sz, A0.ptr, Ai.ptr, Aj.ptr, Ak.ptr, rhs.ptr, ut.ptr, utm1.ptr, float(sc), int(crankNic), st)
    maxIter = int(_f32(cgMaxIterFac) * _f32(max(sx, sy, sz))) * (1 if flags.is3D() else 4)
    res = (ctypes.c_float * 3)()
    none = Grid(s)
    lib.call("mf_cg_solve", sx, sy, sz, flags.ptr, out.ptr, rhs.ptr, residual.ptr, search.ptr, tmp.ptr, A0.ptr, Ai.ptr, Aj.ptr, Ak.ptr,
             none.ptr, PcNone, float(cgAccuracy), int(maxIter), 1, res, st)     # GridCgInterface() : mUseL2Norm(true), conjugategrad.h:31
    _last_cg["iterations"], _last_cg["residual"] = int(res[0]), float(res[1])
    utm1.swap(ut)
    ut.copyFrom(out)


def _uv_offset(offset):
    if offset is None or (isinstance(offset, int) and not isinstance(offset, bool) and offset == 0):
        return (0.0, 0.0, 0.0)                  # (Real)i + 0 is (Real)i: NULL and a zero offset write the same words
    v = _to_vec3(offset)
    return tuple(float(_f32(c)) for c in (v.x, v.y, v.z))


@plugin
def resetUvGrid(target, offset=None):
    """grid.cpp:591-600: every cell takes its own coordinates (plus offset)"""
    _chk(target, VecGrid, "Grid<Vec3>")
    off = _uv_offset(offset)
    s = target.parent
    lib = _extension_lib(s, "resetUvGrid", "fields")
    lib.call("mf_fields_reset_uv", target.sx, target.sy, target.sz, target.ptr, off[0], off[1], off[2], s.stream)


@plugin
def getUvWeight(uv):
    """grid.cpp:576: the x component of cell 0 (one 4-byte read-back)"""
    _chk(uv, VecGrid, "Grid<Vec3>")
    s = uv.parent
    lib = _extension_lib(s, "getUvWeight", "fields")
    out = ctypes.c_float(0.0)
    lib.call("mf_fields_get_uv_weight", uv.ptr, ctypes.byref(out), s.stream)
    return float(out.value)


def _uv_grid_time(t, resetTime):
    """computeUvGridTime, grid.cpp:581-583: fmod(t / resetTime, 1) in fp32 (fmodf is exact)"""
    with np.errstate(all="ignore"):
        return _f32(np.fmod(_f32(t) / _f32(resetTime), _f32(1.0)))


def _uv_ramp(t):
    """computeUvRamp, grid.cpp:585-589: `2. * t` and `2. - w` are double expressions rounded once"""
    w = _f32(2.0 * float(t))
    if float(w) > 1.0:
        w = _f32(2.0 - float(w))
    return w


def _uv_weight_scalars(t, dt, resetTime, index, numUvs):
    """the host half of updateUvWeight, grid.cpp:603-616, in fp32 as written: (weight, reset?)"""
    with np.errstate(all="ignore"):
        t, dt, resetTime = _f32(t), _f32(dt), _f32(resetTime)
        timeOff = resetTime / _f32(numUvs)
        lastt = _uv_grid_time(t + _f32(index) * timeOff - dt, resetTime)
        currt = _uv_grid_time(t + _f32(index) * timeOff, resetTime)
        w = _uv_ramp(currt)
        total = _f32(0.0)
        for i in range(numUvs):
            total = _f32(total + _uv_ramp(_uv_grid_time(t + _f32(i) * timeOff, resetTime)))
        if total <= _f32(1e-6):
            w = _f32(1.0)
        else:
            w = _f32(w / total)
    return w, bool(currt < lastt)


@plugin
def updateUvWeight(resetTime, index, numUvs, uv, offset=None):
    """grid.cpp:601-627: the hat-function weight of uv grid `index` of `numUvs` at the solver's time, normalised over all of them,
    goes into cell 0; the grid is reset when its normalised time wrapped during the last step.  Scalars on the host in fp32, the
    reset and the cell-0 write are kernels."""
    index, numUvs = _coerce(index, 0), _coerce(numUvs, 0)
    _chk(uv, VecGrid, "Grid<Vec3>")
    off = _uv_offset(offset)
    s = uv.parent
    w, reset = _uv_weight_scalars(s.timeTotal, s.getDt(), resetTime, index, numUvs)
    lib = _extension_lib(s, "updateUvWeight", "fields")
    if reset:
        lib.call("mf_fields_reset_uv", uv.sx, uv.sy, uv.sz, uv.ptr, off[0], off[1], off[2], s.stream)
    lib.call("mf_fields_set_uv_weight", uv.n, uv.ptr, float(w), s.stream)


@plugin
def extrapolateSimpleFlags(flags, val, distance=4, flagFrom=_FLAG_FLUID, flagTo=_FLAG_OBSTACLE):
    """waveletturbulence.cpp:239-307: val spreads from the cells with flagFrom into the cells with flagTo, `distance` layers deep,
    each new cell the average of its neighbours of the previous layer.  One mark launch and one launch per layer, in place: the
    reference's serial loop is order-free.  Nothing is read back; without target cells no pass can write."""
    _chk(flags, FlagGrid, "FlagGrid"); _chk(val, GridBase, "GridBase")
    t = val.getType()
    if t & GridBase.TypeReal:
        ncomp, is_int = 1, 0
    elif t & GridBase.TypeInt:
        ncomp, is_int = 1, 1
    elif t & GridBase.TypeVec3:
        ncomp, is_int = 3, 0
    else:
        raise RuntimeError("extrapolateSimpleFlags: Grid Type is not supported (only int, Real, Vec3)")
    s = flags.parent
    lib = _extension_lib(s, "extrapolateSimpleFlags", "fields")
    flags._check_same(val)
    tmp = _scratch_grid(s, core.IntGrid)        # the mark pass writes every cell
    lib.call("mf_fields_extrapolate_mark", flags.n, flags.ptr, tmp.ptr, int(flagFrom), s.stream)
    for d in range(1, 1 + distance):
        lib.call("mf_fields_extrapolate_pass", flags.sx, flags.sy, flags.sz, flags.ptr, tmp.ptr, val.ptr, ncomp, is_int, d, int(flagTo), s.stream)


@plugin
def initVortexVelocity(phiObs, vel, center, radius):
    """initplugins.cpp:478-503, set-up code of test_1040_secOrderBnd.py: a solid-body vortex around `center` in the x and y
    components of every cell with phiObs >= -1.  Host code of the library in fp32 with the C library's sqrtf / atan2f / sinf /
    cosf; phiObs comes down, vel goes down and up again."""
    _chk(phiObs, Grid, "Grid<Real>"); _chk(vel, MACGrid, "MACGrid")
    c = _to_vec3(center)
    s = vel.parent
    lib = _extension_lib(s, "initVortexVelocity", "fields")
    phiObs._check_same(vel)
    s.sync()
    phi = np.ascontiguousarray(phiObs.data.detach().cpu().numpy())
    v = np.ascontiguousarray(vel.data.detach().cpu().numpy()).copy()
    lib.call("mf_fields_vortex_velocity", vel.sx, vel.sy, vel.sz, phi.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p),
             float(_f32(c.x)), float(_f32(c.y)), float(_f32(radius)))
    vel.data.copy_(torch.from_numpy(v).to(vel.data.device))


# ---- mesh level sets as inflow (plugin/initplugins.cpp:132-152): include/open/manta_hip_meshsdf.h -----------------------------------
_mesh_sdf_stats = {"sources": 0, "binned": 0, "rounds": 0}


def lastMeshSdfStats():
    """of the most recent meshSDF (Mesh.computeLevelset / getLevelset / applyMeshToGrid, densityInflowMesh*): `sources` generated,
    `binned` (those inside the grid) and the flood fill's `rounds` (launches; the last one changed nothing)"""
    return dict(_mesh_sdf_stats)


def _inflow_mesh_sdf(name, flags, density, mesh, sigma, cutoff):
    from .core import LevelsetGrid, Mesh
    s = density.parent
    lib = _extension_lib(s, name, "meshsdf")
    _chk(flags, FlagGrid, "FlagGrid")
    if not isinstance(mesh, Mesh):
        raise RuntimeError("can't convert argument to Mesh*")
    if not density.is3D():
        raise RuntimeError("%s: 3-D grids only" % name)
    density._check_same(flags)
    sdf = LevelsetGrid(s)
    mesh._mesh_sdf(lib, name, sdf, sigma, cutoff)
    return lib, sdf


@plugin
def densityInflowMesh(flags, density, mesh, value=1., cutoff=7., sigma=0.):
    """initplugins.cpp:147-152: computeLevelset(sdf, 2., cutoff), then fluid cells with sdf <= sigma take `value`"""
    lib, sdf = _inflow_mesh_sdf("densityInflowMesh", flags, density, mesh, 2., cutoff)
    lib.call("mf_meshsdf_apply_density", flags.sx, flags.sy, flags.sz, flags.ptr, density.ptr, sdf.ptr, float(value), float(sigma),
             density.parent.stream)


@plugin
def densityInflowMeshNoise(flags, density, noise, mesh, scale=1.0, sigma=0.):
    """initplugins.cpp:139-144: computeLevelset(sdf, 1.), then KnApplyNoiseInfl as densityInflow runs it"""
    lib, sdf = _inflow_mesh_sdf("densityInflowMeshNoise", flags, density, mesh, 1., -1.)
    lib.call("mf_density_inflow", flags.sx, flags.sy, flags.sz, flags.ptr, density.ptr, sdf.ptr, _ptr(noise._tile), noise._params(),
             float(scale), float(sigma), density.parent.stream)


# ---- level-set reinitialisation (levelset.cpp:122-228): include/open/manta_hip_reinit.h; the method is LevelsetGrid.reinitMarching ------
_reinit_stats = {"windows": (0, 0), "subrounds": (0, 0), "pops": (0, 0), "serial": (0, 0)}
_reinit_work = {"launches": (0, 0), "readbacks": (0, 0)}      # kernel launches and scalar read-backs of the same call (tools/reinit_time.py)


def lastReinitStats():
    """of the most recent LevelsetGrid.reinitMarching, each a pair (inward march, outward march): `windows` of keys, `subrounds` (a
    selecting and a popping launch each), `pops`, and `serial` (1: the literal loop ran on the host, and windows / subrounds are 0)"""
    return dict(_reinit_stats)


# =========================================================================================================
# 4-D grids (grid4d.cpp:292-467): include/open/manta_hip_grid4d.h; the classes are core.Grid4Real / Grid4Int / Grid4Vec3 / Grid4Vec4
# =========================================================================================================
def _chk4(obj, cls, what):
    if not isinstance(obj, cls):
        raise RuntimeError("can't convert argument to Grid4d<%s>*" % what)
    return obj


def _same4(name, a, b):
    if a.dims != b.dims:
        raise RuntimeError("%s: different Grid4d resolutions [%d,%d,%d,%d] vs [%d,%d,%d,%d]" % ((name,) + a.dims + b.dims))


def _comp4d(name, entry, real, vec, src, dst, c):
    _chk4(real, core.Grid4Real, "Real")
    _chk4(vec, core.Grid4Vec4, "Vec4")
    lib = _extension_lib(real.parent, name, "grid4d")
    _same4(name, src, dst)
    c = int(c)
    if not 0 <= c < 4:
        raise RuntimeError("%s: component %d of a Vec4" % (name, c))
    lib.call(entry, real.n, src.ptr, dst.ptr, c, real.parent.stream)


@plugin
def getComp4d(src, dst, c):
    """knGetComp4d: dst = src[c]"""
    _comp4d("getComp4d", "mf_grid4d_get_comp", dst, src, src, dst, c)


@plugin
def setComp4d(src, dst, c):
    """knSetComp4d: dst[c] = src"""
    _comp4d("setComp4d", "mf_grid4d_set_comp", src, dst, src, dst, c)


def _max_diff4d(name, cls, what, g1, g2):
    _chk4(g1, cls, what)
    _chk4(g2, cls, what)
    lib = _extension_lib(g1.parent, name, "grid4d")
    _same4(name, g1, g2)
    r = ctypes.c_double()
    lib.call("mf_grid4d_max_diff", g1._ncomp, int(g1._is_int), g1.n, g1.ptr, g2.ptr, ctypes.byref(r), g1.parent.stream)
    return float(np.float32(r.value))        # the plugin returns a Real


@plugin
def grid4dMaxDiff(g1, g2):
    """the largest |g1 - g2| (grid4d.cpp:352-359)"""
    return _max_diff4d("grid4dMaxDiff", core.Grid4Real, "Real", g1, g2)


@plugin
def grid4dMaxDiffInt(g1, g2):
    return _max_diff4d("grid4dMaxDiffInt", core.Grid4Int, "int", g1, g2)


@plugin
def grid4dMaxDiffVec3(g1, g2):
    """the largest per-cell sum of the component differences, formed in fp64 (grid4d.cpp:368-379)"""
    return _max_diff4d("grid4dMaxDiffVec3", core.Grid4Vec3, "Vec3", g1, g2)


@plugin
def grid4dMaxDiffVec4(g1, g2):
    return _max_diff4d("grid4dMaxDiffVec4", core.Grid4Vec4, "Vec4", g1, g2)


def _set_region4d(name, dst, start, end, v):
    lib = _extension_lib(dst.parent, name, "grid4d")
    s, e = core._to_vec4(start), core._to_vec4(end)
    lib.call("mf_grid4d_set_region", dst.sx, dst.sy, dst.sz, dst.st, dst.ptr, dst._ncomp, s.x, s.y, s.z, s.t, e.x, e.y, e.z, e.t,
             v[0], v[1], v[2], v[3], dst.parent.stream)


@plugin
def setRegion4d(dst, start, end, value):
    """knSetRegion4d<Real>: cells with start <= (i, j, k, t) <= end, compared as floats, take the value"""
    _chk4(dst, core.Grid4Real, "Real")
    _set_region4d("setRegion4d", dst, start, end, (float(value), 0., 0., 0.))


@plugin
def setRegion4dVec4(dst, start, end, value):
    _chk4(dst, core.Grid4Vec4, "Vec4")
    _set_region4d("setRegion4dVec4", dst, start, end, tuple(core._to_vec4(value)))


@plugin
def getSliceFrom4d(src, srct, dst):
    """dst(i, j, k) = src(i, j, k, srct) where both grids have the cell; an srct outside the grid changes nothing"""
    _chk4(src, core.Grid4Real, "Real")
    _chk(dst, Grid, "Grid<Real>")
    lib = _extension_lib(src.parent, "getSliceFrom4d", "grid4d")
    _extension_lib(dst.parent, "getSliceFrom4d", "grid4d")
    lib.call("mf_grid4d_get_slice", src.sx, src.sy, src.sz, src.st, src.ptr, 1, int(srct), dst.sx, dst.sy, dst.sz, dst.ptr, None,
             src.parent.stream)


@plugin
def getSliceFrom4dVec(src, srct, dst, dstt=None):
    """the x, y, z of the slice into a Vec3 grid, the fourth component into dstt where that is given"""
    _chk4(src, core.Grid4Vec4, "Vec4")
    _chk(dst, VecGrid, "Grid<Vec3>")
    dstt = _opt(dstt, Grid, "Grid<Real>")
    lib = _extension_lib(src.parent, "getSliceFrom4dVec", "grid4d")
    _extension_lib(dst.parent, "getSliceFrom4dVec", "grid4d")
    if dstt is not None:
        dst._check_same(dstt)
    lib.call("mf_grid4d_get_slice", src.sx, src.sy, src.sz, src.st, src.ptr, 4, int(srct), dst.sx, dst.sy, dst.sz, dst.ptr,
             None if dstt is None else dstt.ptr, src.parent.stream)


def grid_factor_4d(s1, s2, offset, scale, size):
    """gridFactor4d, grid4d.cpp:440-444, in fp32 as the reference's Vec4 arithmetic: the source factor and the offset of knInterpol4d"""
    f32 = np.float32
    s1, s2 = np.array(s1, f32), np.array(s2, f32)
    off, scale, size = (np.array(tuple(core._to_vec4(v)), f32) for v in (offset, scale, size))
    s2 = np.where(size > 0., size, s2)
    fac = (s1 / s2) / scale
    return fac, -off * fac + fac * f32(0.5)


def _interpolate4d(name, cls, what, target, source, offset, scale, size):
    _chk4(target, cls, what)
    _chk4(source, cls, what)
    lib = _extension_lib(target.parent, name, "grid4d")
    _extension_lib(source.parent, name, "grid4d")
    if min(source.dims) < 2:
        raise RuntimeError("%s: every axis of the source needs 2 cells, got [%d,%d,%d,%d]" % ((name,) + source.dims))
    if target is source:
        raise RuntimeError("%s: target and source are the same grid" % name)
    with np.errstate(all="ignore"):
        fac, off = grid_factor_4d(source.dims, target.dims, offset, scale, size)
    lib.call("mf_grid4d_interpolate", target.sx, target.sy, target.sz, target.st, target.ptr, source.sx, source.sy, source.sz, source.st,
             source.ptr, target._ncomp, *[float(x) for x in fac], *[float(x) for x in off], target.parent.stream)


@plugin
def interpolateGrid4d(target, source, offset=core.vec4(0.), scale=core.vec4(1.), size=core.vec4(-1.)):
    """linear interpolation of a 4-D Real grid to another size (grid4d.cpp:455-460)"""
    _interpolate4d("interpolateGrid4d", core.Grid4Real, "Real", target, source, offset, scale, size)


@plugin
def interpolateGrid4dVec(target, source, offset=core.vec4(0.), scale=core.vec4(1.), size=core.vec4(-1.)):
    _interpolate4d("interpolateGrid4dVec", core.Grid4Vec4, "Vec4", target, source, offset, scale, size)


# ---- particle-data plugins of the test harness (plugin/initplugins.cpp:53-64, 287-294) and its three grid helpers (:189-269, flip.cpp:191) ----
def _set_noise_pdata(name, kind, cls, what, parts, pd, noise, scale):
    if not isinstance(parts, core.BasicParticleSystem):
        raise RuntimeError("can't convert argument to BasicParticleSystem*")
    if not isinstance(pd, cls):
        raise RuntimeError("can't convert argument to ParticleDataImpl<%s>*" % what)
    s = parts.parent
    lib = _extension_lib(s, name, "grid4d")
    if pd.sys is not parts:
        raise RuntimeError("%s: the channel belongs to another particle system" % name)
    lib.call("mf_grid4d_pdata_set_noise", kind, parts.np, pd.cap, pd.ptr, parts.cap, _ptr(parts.pos), _ptr(noise._tile), noise._params(),
             float(scale), s.stream)


@plugin
def setNoisePdata(parts, pd, noise, scale=1.):
    """knSetPdataNoise<Real>: pd = noise.evaluate(pos) * scale in every slot"""
    _set_noise_pdata("setNoisePdata", 0, core.PdataReal, "Real", parts, pd, noise, scale)


@plugin
def setNoisePdataVec3(parts, pd, noise, scale=1.):
    """knSetPdataNoiseVec<Vec3>: pd = noise.evaluateVec(pos) * scale"""
    _set_noise_pdata("setNoisePdataVec3", 2, core.PdataVec3, "Vec3", parts, pd, noise, scale)


@plugin
def setNoisePdataInt(parts, pd, noise, scale=1.):
    """knSetPdataNoise<int>: the Real result converted as C does, toward zero"""
    _set_noise_pdata("setNoisePdataInt", 1, core.PdataInt, "int", parts, pd, noise, scale)


@plugin
def addTestParts(parts, num):
    """`num` buffered particles at the origin, doCompress(), insertBufferedParticles() (initplugins.cpp:287-294)"""
    if not isinstance(parts, core.BasicParticleSystem):
        raise RuntimeError("can't convert argument to BasicParticleSystem*")
    parts.doCompress()
    parts.insertBufferedParticles(np.zeros((max(int(num), 0), 3), np.float32))


def _check_symmetry(name, a, err, symmetrize, axis, bound, disable, mac):
    err = _opt(err, Grid, "Grid<Real>")
    s = a.parent
    lib = _extension_lib(s, name, "grid4d")
    if err is not None:
        a._check_same(err)
    if axis not in (0, 1, 2):
        raise RuntimeError("%s: axis %d" % (name, axis))
    lib.call("mf_grid4d_check_symmetry", a.sx, a.sy, a.sz, a.ptr, mac, None if err is None else err.ptr, int(symmetrize), axis, bound,
             disable, s.stream)


@plugin
def checkSymmetry(a, err=None, symmetrize=False, axis=0, bound=0):
    """err = |a - mirror of a about the middle of `axis`|; with symmetrize the lower half takes the upper half's values"""
    _chk(a, Grid, "Grid<Real>")
    _check_symmetry("checkSymmetry", a, err, symmetrize, axis, bound, 0, 0)


@plugin
def checkSymmetryVec3(a, err=None, symmetrize=False, axis=0, bound=0, disable=0):
    """the MAC form: the normal component is mirrored about size + 1 with its sign flipped, the other two like a scalar; err adds up"""
    _chk(a, VecGrid, "Grid<Vec3>")
    _check_symmetry("checkSymmetryVec3", a, err, symmetrize, axis, bound, disable, 1)


@plugin
def testInitGridWithPos(grid):
    """grid(i, j, k) = norm(Vec3(i, j, k)) (flip.cpp:191-193)"""
    _chk(grid, Grid, "Grid<Real>")
    lib = _extension_lib(grid.parent, "testInitGridWithPos", "grid4d")
    lib.call("mf_grid4d_init_grid_with_pos", grid.sx, grid.sy, grid.sz, grid.ptr, grid.parent.stream)


# =========================================================================================================
# vortex particles (plugin/vortexplugins.cpp:29-37, 169-189, 298-310): include/open/manta_hip_vortex.h; the class is
# core.VortexParticleSystem.  The vortex sheet half of the file (VortexSheetMesh) is not implemented.
# =========================================================================================================
def _chk_shape(shape):
    if not (hasattr(shape, "_inside") and hasattr(shape, "_inside_centres")):
        raise RuntimeError("can't convert argument to Shape*")
    return shape


@plugin
def VPseedK41(system, shape, strength=0.0, sigma0=0.2, sigma1=1.0, probability=1.0, N=3.0):
    """vortexplugins.cpp:169-189 (host, every backend): the cells of the system's solver in FOR_IJK order; one draw of the process-wide
    stream per cell inside the shape, and seven more -- p, then the direction and the position offset, each drawn z, y, x (the
    reference compiler's argument evaluation order) -- where the draw is below probability * dt.  powf / pow / normalize run in the C
    library (core._seed_k41_host)."""
    f32 = np.float32
    if not isinstance(system, core.VortexParticleSystem):
        raise RuntimeError("can't convert argument to VortexParticleSystem*")
    _chk_shape(shape)
    s = system.parent
    sx, sy, sz = s.mGridSize
    thr = f32(f32(probability) * f32(s.getDt()))
    cells = np.nonzero(np.asarray(shape._inside_centres(s)).reshape(-1))[0]
    st = core._vortex_seed_stream
    r = st.peek(8 * cells.size)
    hit_cell, hit_at, at = [], [], 0
    below = (r < thr).tolist()
    for c in cells.tolist():
        if below[at]:
            hit_cell.append(c)
            hit_at.append(at + 1)
            at += 8
        else:
            at += 1
    st_r = r[:at].copy()
    st.advance(at)
    hit_cell, hit_at = np.array(hit_cell, np.int64), np.array(hit_at, np.int64)
    draws = st_r[hit_at[:, None] + np.arange(7)[None, :]] if hit_at.size else np.zeros((0, 7), f32)
    p, dirs, off = draws[:, 0], draws[:, 3:0:-1], draws[:, 6:3:-1]
    ijk = np.stack([hit_cell % sx, (hit_cell // sx) % sy, hit_cell // (sx * sy)], 1).astype(f32)
    sigma, vort = core._seed_k41_host(s.lib, f32(strength), f32(sigma0), f32(sigma1), f32(N), p, dirs)
    system._append((ijk + off).astype(f32), vort, sigma)


@plugin
def markAsFixed(mesh, shape, exclusive=True):
    """vortexplugins.cpp:29-37 (host): nodes inside the shape get NfFixed; with `exclusive` the others lose it"""
    if not isinstance(mesh, core.Mesh):
        raise RuntimeError("can't convert argument to Mesh*")
    _chk_shape(shape)
    if mesh.nn == 0:
        return
    pos, _, fl = mesh.nodes_numpy()
    inside = np.asarray(shape._inside(pos[:, 0], pos[:, 1], pos[:, 2]))
    fl = np.where(inside, fl | core.Mesh.NfFixed, (fl & ~core.Mesh.NfFixed) if exclusive else fl).astype(np.int32)
    mesh.nflag[:mesh.nn] = torch.from_numpy(fl).to(mesh.nflag.device)


# =========================================================================================================
# mesh smoothing and component removal (plugin/meshplugins.cpp:36-104, 563-619): include/open/manta_hip_meshops.h, DESIGN.md section 26.
# Both rest on the connectivity tables of core.Mesh._connectivity.  subdivideMesh is not implemented.
# =========================================================================================================
_meshops_stats = {}


def lastMeshOpsStats():
    """of the most recent connectivity build, smoothMesh or killSmallComponents: `singletons` / `multi` (edge groups of one corner / of
    three or more), `rebuilt` (False: the cached tables were reused); after killSmallComponents `rounds` of labelling, `components`,
    `nodes` and `tris` deleted; after smoothMesh `sums`, the 2 x 4 fp64 sums of computeCenterOfMass before and after the steps"""
    return dict(_meshops_stats)


def _real_arg(v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise RuntimeError("argument is not a float")
    return float(np.float32(v))


def _meshops_args(name, mesh):
    if not isinstance(mesh, core.Mesh):
        raise RuntimeError("can't convert argument to Mesh*")
    return _extension_lib(mesh.parent, name, "meshops")


@plugin
def smoothMesh(mesh, strength, steps=1, minLength=1e-5):
    """meshplugins.cpp:36-104: `steps` Jacobi sweeps over the 1-rings (one lane per node, ring walked ascending), then the rescale about
    the centre of mass that restores the volume; the two centres of mass are fixed-tree fp64 sums read back as 2 x 32 bytes"""
    lib = _meshops_args("smoothMesh", mesh)
    strength, minLength = _real_arg(strength), _real_arg(minLength)
    s = mesh.parent
    str_ = float(min(np.float32(np.float32(s.getDt()) * np.float32(strength)), np.float32(1)))
    conn = mesh._connectivity(lib, "smoothMesh")
    _meshops_stats.pop("rounds", None)
    need = ctypes.c_int64(0)
    lib.call("mf_meshops_tmp_bytes", mesh.nt, mesh.nn, ctypes.byref(need))
    tmp, release = mesh._meshops_scratch(need.value)
    temp, release_temp = mesh._meshops_scratch(12 * max(mesh.nn, 1))
    try:
        def sums():
            out = (ctypes.c_double * 4)()
            lib.call("mf_meshops_volume_sums", mesh.nt, mesh.tcap, _ptr(mesh.tri), mesh.nn, mesh.ncap, _ptr(mesh.pos), _ptr(tmp),
                     tmp.numel() * tmp.element_size(), out, s.stream)
            return out
        s0 = sums()
        for _ in range(steps):
            lib.call("mf_meshops_smooth_step", mesh.nn, mesh.ncap, _ptr(mesh.pos), _ptr(mesh.nflag), _ptr(conn["nodeOff"]), _ptr(conn["nodes"]),
                     _ptr(conn["triOff"]), str_, minLength, _ptr(temp), s.stream)
        s1 = sums()
        sc = (ctypes.c_float * 7)()
        lib.call("mf_meshops_rescale_scalars", s0, s1, sc)
        lib.call("mf_meshops_rescale", mesh.nn, mesh.ncap, _ptr(mesh.pos), _ptr(mesh.nflag), sc[0], sc[1], sc[2], sc[3], sc[4], sc[5], sc[6], s.stream)
        _meshops_stats["sums"] = (tuple(s0), tuple(s1))
    finally:
        release_temp()
        release()


@plugin
def killSmallComponents(mesh, elements=10):
    """meshplugins.cpp:563-619: the components of the triangle graph with fewer than `elements` triangles are removed with their nodes,
    in the reference's order (removeTri over the tainted triangles descending, removeNodes over the nodes in order of first appearance).
    Two refusals leave the mesh untouched where the reference does not: an edge with three or more triangles, and a node that a
    killed and a kept component share."""
    lib = _meshops_args("killSmallComponents", mesh)
    s = mesh.parent
    conn = mesh._connectivity(lib, "killSmallComponents")
    if conn["multi"]:
        raise RuntimeError("killSmallComponents: non-manifold edge")
    need = ctypes.c_int64(0)
    lib.call("mf_meshops_tmp_bytes", mesh.nt, mesh.nn, ctypes.byref(need))
    tmp, release = mesh._meshops_scratch(need.value)
    try:
        out = (ctypes.c_int32 * 5)()
        nbytes = tmp.numel() * tmp.element_size()
        lib.call("mf_meshops_kill_plan", mesh.nt, mesh.tcap, _ptr(mesh.tri), mesh.nn, _ptr(conn["opposite"]), elements, _ptr(tmp), nbytes, out, s.stream)
        rounds, comps, ktris, knodes, shared = (int(x) for x in out)
        if shared >= 0:
            raise RuntimeError("killSmallComponents: node %d is shared with a kept component" % shared)
        _meshops_stats.pop("sums", None)
        _meshops_stats.update(rounds=rounds, components=comps, tris=ktris, nodes=knodes)
        if ktris == 0:
            return
        lib.call("mf_meshops_kill_apply", mesh.nt, mesh.tcap, _ptr(mesh.tri), _ptr(mesh.tflag), mesh.nn, mesh.ncap, _ptr(mesh.pos), _ptr(mesh.normal),
                 _ptr(mesh.nflag), ktris, knodes, _ptr(tmp), nbytes, s.stream)
        mesh.nt, mesh.nn = mesh.nt - ktris, mesh.nn - knodes
        mesh._topo_gen += 1
    finally:
        release()
    from . import api
    api.mantaMsg("Killed small components : %d nodes, %d tris deleted." % (knodes, ktris), 0)      # the reference writes to cout: every debug level


@plugin
def densityFromLevelset(phi, density, value=1.0, sigma=1.0):
    """vortexplugins.cpp:298-310, one kernel: a linear ramp of width sigma over the interface, 0 in the two outermost layers of every
    axis (on a 2-D solver that is every cell, as in the reference)"""
    s = phi.parent if isinstance(phi, GridBase) else density.parent
    lib = _extension_lib(s, "densityFromLevelset", "vortex")
    _chk(phi, LevelsetGrid, "LevelsetGrid"); _chk(density, Grid, "Grid<Real>")
    phi._check_same(density)
    lib.call("mf_vortex_density_from_levelset", phi.sx, phi.sy, phi.sz, phi.ptr, density.ptr, float(np.float32(value)), float(np.float32(sigma)),
             s.stream)


# =========================================================================================================
# the array bridge and the MLFLIP data plugins (plugin/numpyconvert.cpp:29-223, plugin/tfplugins.cpp:22-220):
# include/open/manta_hip_mlflip.h.  An array is a numpy ndarray, a CPU tensor or a tensor on the solver's device; a device tensor
# is read or written where it is, on the solver's stream, a host array goes through one device staging tensor.  Every plugin is
# refused first (z-slab solver, backend without the extension), validates second and touches memory third.  DESIGN.md section 22.
# =========================================================================================================
_NP_TYPES = {np.dtype(np.int32): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2}
_TORCH_TYPES = {torch.int32: 0, torch.float32: 1, torch.float64: 2}
_TYPE_NAMES = ("int32", "float32", "float64")
_TORCH_OF = (torch.int32, torch.float32, torch.float64)


def _mlflip_lib(name, *objs):
    """the library for plugin `name`, found through the first argument that has a solver; the refusals come before every other check"""
    for o in objs:
        if isinstance(o, core.PbClass):
            return o.parent, _extension_lib(o.parent, name, "mlflip")
    raise RuntimeError("%s: can't convert argument to a grid or particle object" % name)


def _solver_device(s):
    d = torch.device(s.device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


class _Array(object):
    """one validated array argument: `code` (0 int32, 1 float32, 2 float64), `size` and `dims` as the reference's PyArrayContainer
    has them.  stage() gives the device tensor the kernel reads or writes, finish() brings a host target home."""

    def __init__(self, who, s, obj, target, host, code):
        self.who, self.s, self.obj, self.target, self.host, self.code = who, s, obj, target, host, code
        self.dims = tuple(int(v) for v in obj.shape)
        self.size = int(obj.size) if isinstance(obj, np.ndarray) else int(obj.numel())
        self.dev = None

    def stage(self, keep=False):
        """keep: a target the kernel writes only partly starts from the caller's values"""
        dev = _solver_device(self.s)
        if not self.host:
            self.dev = self.obj if self.target else self.obj.contiguous()
        elif self.target and not keep:
            self.dev = torch.empty(self.size, dtype=_TORCH_OF[self.code], device=dev)
        else:
            if isinstance(self.obj, np.ndarray):
                h = np.ascontiguousarray(self.obj)       # as PyArray_CheckFromAny does in the reference
                h = torch.from_numpy(h if h.flags["WRITEABLE"] else h.copy())
            else:
                h = self.obj.contiguous()
            self.dev = h.reshape(-1).to(dev)
        return _ptr(self.dev)

    def finish(self):
        if self.target and self.host:
            h = torch.from_numpy(self.obj) if isinstance(self.obj, np.ndarray) else self.obj
            h.view(-1).copy_(self.dev.view(-1))      # a blocking download on the solver's stream


def _array_arg(who, s, obj, target, need=None):
    """Validate the array argument of plugin `who` on solver `s` and return its _Array; nothing is copied or staged here.
    target: the plugin writes it (it must then be C-contiguous and writable); need: the one element type the plugin takes, where the
    reference reinterprets the memory blindly."""
    if isinstance(obj, np.ndarray):
        code, host = _NP_TYPES.get(obj.dtype), True
        contiguous, found = obj.flags["C_CONTIGUOUS"], str(obj.dtype)
        if target and not obj.flags["WRITEABLE"]:
            raise RuntimeError("%s: target array is read-only" % who)
    elif isinstance(obj, torch.Tensor):
        code, host = _TORCH_TYPES.get(obj.dtype), obj.device.type == "cpu"
        contiguous, found = obj.is_contiguous(), str(obj.dtype).replace("torch.", "")
        if not host and obj.device != _solver_device(s):
            raise RuntimeError("%s: the tensor lives on %s, the solver on %s" % (who, obj.device, _solver_device(s)))
    else:
        raise RuntimeError("%s: can't convert argument to a numpy array or a torch tensor" % who)
    if need is not None and code != need:
        raise RuntimeError("%s: array of type %s where %s is needed" % (who, found, _TYPE_NAMES[need]))
    if code is None:
        raise RuntimeError("%s: unknown type of Numpy array" % who)      # numpyWrap.cpp:74-88
    if target and not contiguous:
        raise RuntimeError("%s: target array must be C-contiguous" % who)
    return _Array(who, s, obj, target, host, code)


def _check_grid_array(who, a, g, to_grid):
    """the two assertions of copyArrayToGrid* / copyGridToArray* (numpyconvert.cpp:38-39, 64-65, 94-95, 121-122), with the array's
    element type checked first: the reference would zero the target grid and then fail"""
    vec = g._ncomp == 3
    if vec and a.code == 0:
        raise RuntimeError("%s: unknown/unsupported type of Vec3 Numpy array" % who)
    if a.size != g._ncomp * g.n:
        if vec:
            raise RuntimeError("%s: The size of the numpy array doesn't match the size of the grid!" % who)
        if to_grid:
            raise RuntimeError("%s: The size of the numpy array doesn't match the size of the Grid!" % who)
        raise RuntimeError("%s: The size of the numpy array %d doesn't match the size of the grid!" % (who, a.size))
    if a.dims[:3] != (g.sz, g.sy, g.sx):
        d = a.dims + (0, 0, 0)
        arr, grd = "(%d, %d, %d)" % (d[2], d[1], d[0]), "(%d, %d, %d)" % (g.sx, g.sy, g.sz)
        if to_grid:
            raise RuntimeError("%s: The dimensions of source numpy array %s and target grid %s do not match!" % (who, arr, grd))
        raise RuntimeError("%s: The dimensions of source grid %s and target numpy array %s do not match!" % (who, grd, arr))


def _array_to_grid(who, source, target, cls, cname):
    s, lib = _mlflip_lib(who, target)
    _chk(target, cls, cname)
    a = _array_arg(who, s, source, False)
    _check_grid_array(who, a, target, True)
    if target._ncomp == 3:
        lib.call("mf_mlflip_elements_to_planes", target.n, target.n, a.stage(), a.code, target.ptr, s.stream)
    else:
        lib.call("mf_mlflip_convert", target.n, a.stage(), a.code, target.ptr, 0 if target._kind == "int" else 1, s.stream)


def _grid_to_array(who, source, target, cls, cname):
    s, lib = _mlflip_lib(who, source)
    _chk(source, cls, cname)
    a = _array_arg(who, s, target, True)
    _check_grid_array(who, a, source, False)
    if source._ncomp == 3:
        lib.call("mf_mlflip_planes_to_elements", source.n, source.n, source.ptr, a.stage(), a.code, s.stream)
    else:
        lib.call("mf_mlflip_convert", source.n, source.ptr, 0 if source._kind == "int" else 1, a.stage(), a.code, s.stream)
    a.finish()


@plugin
def copyArrayToGridReal(source, target):
    """numpyconvert.cpp:145-147: int32 / float32 / float64 [z][y][x] (or [z][y][x][1]) into a real grid, converted as C does"""
    _array_to_grid("copyArrayToGridReal", source, target, Grid, "Grid<Real>")


@plugin
def copyGridToArrayReal(source, target):
    _grid_to_array("copyGridToArrayReal", source, target, Grid, "Grid<Real>")


@plugin
def copyArrayToGridFlag(source, target):
    """a float array truncates towards zero"""
    _array_to_grid("copyArrayToGridFlag", source, target, FlagGrid, "FlagGrid")


@plugin
def copyGridToArrayFlag(source, target):
    _grid_to_array("copyGridToArrayFlag", source, target, FlagGrid, "FlagGrid")


@plugin
def copyArrayToGridLevelset(source, target):
    _array_to_grid("copyArrayToGridLevelset", source, target, LevelsetGrid, "LevelsetGrid")


@plugin
def copyGridToArrayLevelset(source, target):
    _grid_to_array("copyGridToArrayLevelset", source, target, LevelsetGrid, "LevelsetGrid")


@plugin
def copyArrayToGridVec3(source, target):
    """float32 / float64 [z][y][x][3] into the three component planes: one transposing kernel"""
    _array_to_grid("copyArrayToGridVec3", source, target, VecGrid, "Grid<Vec3>")


@plugin
def copyGridToArrayVec3(source, target):
    _grid_to_array("copyGridToArrayVec3", source, target, VecGrid, "Grid<Vec3>")


@plugin
def copyArrayToGridMAC(source, target):
    _array_to_grid("copyArrayToGridMAC", source, target, MACGrid, "MACGrid")


@plugin
def copyGridToArrayMAC(source, target):
    _grid_to_array("copyGridToArrayMAC", source, target, MACGrid, "MACGrid")


def _pdata_copy(who, arr, pd, cls, cname, to_pdata):
    """numpyconvert.cpp:189-223: the words of the live slots, no conversion -- so the element type is required (the reference
    reinterprets whatever it is given)"""
    s, lib = _mlflip_lib(who, pd)
    _chk(pd, cls, cname)
    a = _array_arg(who, s, arr, not to_pdata, 0 if pd._dtype == torch.int32 else 1)
    n = pd.size()
    if a.size != n * pd._ncomp:
        raise RuntimeError("%s: The size of the numpy array doesn't match the size of the pdata field!" % who)
    if n == 0:
        return
    if pd._ncomp == 3:
        if to_pdata:
            lib.call("mf_mlflip_elements_to_planes", n, pd.cap, a.stage(), 1, pd.ptr, s.stream)
        else:
            lib.call("mf_mlflip_planes_to_elements", n, pd.cap, pd.ptr, a.stage(), 1, s.stream)
    elif to_pdata:
        lib.call("mf_mlflip_convert", n, a.stage(), a.code, pd.ptr, a.code, s.stream)
    else:
        lib.call("mf_mlflip_convert", n, pd.ptr, a.code, a.stage(), a.code, s.stream)
    a.finish()


@plugin
def copyArrayToPdataInt(source, target):
    _pdata_copy("copyArrayToPdataInt", source, target, core.PdataInt, "ParticleDataImpl<int>", True)


@plugin
def copyPdataToArrayInt(source, target):
    _pdata_copy("copyPdataToArrayInt", target, source, core.PdataInt, "ParticleDataImpl<int>", False)


@plugin
def copyArrayToPdataReal(source, target):
    _pdata_copy("copyArrayToPdataReal", source, target, core.PdataReal, "ParticleDataImpl<Real>", True)


@plugin
def copyPdataToArrayReal(source, target):
    _pdata_copy("copyPdataToArrayReal", target, source, core.PdataReal, "ParticleDataImpl<Real>", False)


@plugin
def copyArrayToPdataVec3(source, target):
    _pdata_copy("copyArrayToPdataVec3", source, target, core.PdataVec3, "ParticleDataImpl<Vec3>", True)


@plugin
def copyPdataToArrayVec3(source, target):
    _pdata_copy("copyPdataToArrayVec3", target, source, core.PdataVec3, "ParticleDataImpl<Vec3>", False)


def _feature_layout(who, np_, is3d, kind, N_row, off_begin, window, fv_size):
    """the checks of a feature call -> (stencil points, values per point)"""
    if window < 0:
        raise RuntimeError("%s: window %d" % (who, window))
    w = 2 * window + 1
    nst, D = w * w * (w if is3d else 1), ((3 if is3d else 2) if kind == 0 else 1)
    if off_begin < 0 or off_begin + nst * D > N_row:
        raise RuntimeError("%s: %d stencil points of %d values from column %d do not fit a row of %d" % (who, nst, D, off_begin, N_row))
    if fv_size < np_ * N_row:
        raise RuntimeError("%s: the feature array holds %d values, %d rows of %d need %d" % (who, fv_size, np_, N_row, np_ * N_row))
    return nst, D


def _extract_feature(who, kind, fv, N_row, off_begin, p, grid, cls, cname, scale, ptype, exclude, window):
    s, lib = _mlflip_lib(who, p, grid)
    if not isinstance(p, core.BasicParticleSystem):
        raise RuntimeError("can't convert argument to BasicParticleSystem*")
    _chk(grid, cls, cname)
    ptype = _opt(ptype, core.PdataInt, "ParticleDataImpl<int>")
    N_row, off_begin = int(N_row), int(off_begin)
    a = _array_arg(who, s, fv, True, 1)
    _feature_layout(who, p.np, grid.is3D(), kind, N_row, off_begin, window, a.size)
    if ptype is not None and ptype.size() != p.np:
        raise RuntimeError("%s: ptype has %d entries, the system %d particles" % (who, ptype.size(), p.np))
    if p.np == 0:
        return
    (np_, cap, pos, pfl), pt = _pargs(p, ptype)
    if ptype is not None and ptype.cap != cap:
        raise RuntimeError("%s: ptype is not a channel of the particle system" % who)
    lib.call("mf_mlflip_extract_feature", kind, grid.sx, grid.sy, grid.sz, grid.ptr, np_, cap, pos, pfl, pt, int(exclude), int(window),
             float(np.float32(scale)), a.stage(keep=True), a.size, N_row, off_begin, s.stream)
    a.finish()


@plugin
def extractFeatureVel(fv, N_row, off_begin, p, vel, scale=1.0, ptype=None, exclude=0, window=1):
    """tfplugins.cpp:38-66, 122-130: interpolMAC(pos + (i, j, k)) * scale for the (2 window + 1)^dim stencil points, i outer, k inner,
    into fv[idx * N_row + off_begin + stencil * D + c]; rows of deleted or excluded slots and the rest of a row are not written"""
    _extract_feature("extractFeatureVel", 0, fv, N_row, off_begin, p, vel, MACGrid, "MACGrid", scale, ptype, exclude, window)


@plugin
def extractFeaturePhi(fv, N_row, off_begin, p, phi, scale=1.0, ptype=None, exclude=0, window=1):
    """tfplugins.cpp:68-93, 131-139: interpol(pos + (i, j, k)) * scale, one value per stencil point"""
    _extract_feature("extractFeaturePhi", 1, fv, N_row, off_begin, p, phi, Grid, "Grid<Real>", scale, ptype, exclude, window)


@plugin
def extractFeatureGeo(fv, N_row, off_begin, p, flag, scale=1.0, ptype=None, exclude=0, window=1):
    """tfplugins.cpp:95-120, 140-148: float(flags at the cell pos + (i, j, k) truncates to) * scale.  Precondition: that cell is inside
    the grid (the reference indexes unchecked; the kernel clamps the cell index)"""
    _extract_feature("extractFeatureGeo", 2, fv, N_row, off_begin, p, flag, FlagGrid, "FlagGrid", scale, ptype, exclude, window)


def _regions(who, r, flags, ctype, counts):
    s, lib = _mlflip_lib(who, r, flags)
    _chk(r, core.IntGrid, "Grid<int>"); _chk(flags, FlagGrid, "FlagGrid")
    flags._check_same(r)
    if r is flags:
        raise RuntimeError("%s: r and flags are the same grid" % who)
    n = ctypes.c_int32(0)
    lib.call("mf_mlflip_regions", flags.sx, flags.sy, flags.sz, flags.ptr, _c_int32(ctype), counts, r.ptr, ctypes.byref(n), s.stream)
    return int(n.value)


def _c_int32(v):
    """an int parameter as the C int it is in the reference (flag masks may have the sign bit)"""
    return ctypes.c_int32(int(v) & 0xffffffff).value


@plugin
def getRegions(r, flags, ctype):
    """tfplugins.cpp:155-176: r = the number (from 1, in the order of their lowest flat index) of the face-connected component of
    flags & ctype cells a cell belongs to, 0 outside; returns the number of components.  Precondition: no ctype cell in the outermost
    layer of the grid (there the reference's flood fill reads across row ends); a neighbour outside the grid is not connected here"""
    return _regions("getRegions", r, flags, ctype, 0)


@plugin
def getRegionalCounts(r, flags, ctype):
    """tfplugins.cpp:178-188: r = the number of cells of the cell's component, 0 outside"""
    _regions("getRegionalCounts", r, flags, ctype, 1)


@plugin
def extendRegion(flags, region, exclude, depth):
    """tfplugins.cpp:190-207: `depth` rounds; a cell without flags & exclude beside a cell with flags & region becomes `region`"""
    s, lib = _mlflip_lib("extendRegion", flags)
    _chk(flags, FlagGrid, "FlagGrid")
    depth = _coerce(depth, 0)
    if depth <= 0:
        return
    tmp = _scratch_grid(s, core.IntGrid)
    lib.call("mf_mlflip_extend_region", flags.sx, flags.sy, flags.sz, flags.ptr, tmp.ptr, _c_int32(region), _c_int32(exclude), depth, s.stream)


@plugin
def markSmallRegions(flags, rcnt, mark, exclude, th=1):
    """tfplugins.cpp:209-220: flags = mark where !(flags & exclude) and rcnt <= th"""
    s, lib = _mlflip_lib("markSmallRegions", flags, rcnt)
    _chk(flags, FlagGrid, "FlagGrid"); _chk(rcnt, core.IntGrid, "Grid<int>")
    flags._check_same(rcnt)
    lib.call("mf_mlflip_mark_small_regions", flags.sx, flags.sy, flags.sz, flags.ptr, rcnt.ptr, _c_int32(mark), _c_int32(exclude), int(th), s.stream)


@plugin
def simpleNumpyTest(grid, npAr, scale):
    """tfplugins.cpp:22-33: grid(i, j, k) += scale * npAr[j * sx + i]; the array is float32 and holds at least sx * sy values (the
    reference checks neither)"""
    s, lib = _mlflip_lib("simpleNumpyTest", grid)
    _chk(grid, Grid, "Grid<Real>")
    a = _array_arg("simpleNumpyTest", s, npAr, False, 1)
    if a.size < grid.sx * grid.sy:
        raise RuntimeError("simpleNumpyTest: the array holds %d values, a plane of the grid has %d" % (a.size, grid.sx * grid.sy))
    lib.call("mf_mlflip_simple_array_add", grid.sx, grid.sy, grid.sz, grid.ptr, a.stage(), a.size, float(np.float32(scale)), s.stream)


# =========================================================================================================
# the smoke data-generation plugins: the Gaussian grid blurs, calcCenterOfMass and projectPpmFull of source/plugin/initplugins.cpp
# (:273-282, :337-348, :510-655; util/simpleimage.cpp) and getLaplacian / getCurvature of source/plugin/flip.cpp:779-785:
# include/open/manta_hip_datagen.h, whole-domain solvers only.  Every plugin is refused first (z-slab solver, backend without the
# extension), validates second and touches memory third.  DESIGN.md section 23.
# =========================================================================================================
def _datagen_lib(name, *objs):
    """the solver and its library for plugin `name`, found through the first argument that is a grid"""
    for o in objs:
        if isinstance(o, core.PbClass):
            return o.parent, _extension_lib(o.parent, name, "datagen")
    raise RuntimeError("%s: can't convert argument to a grid" % name)


def _blur(name, cls, cname, kind, ncomp, oG, tG, si):
    s, lib = _datagen_lib(name, oG, tG)
    _chk(oG, cls, cname); _chk(tG, cls, cname)
    oG._check_same(tG)
    sigma = np.float32(si)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError("%s: sigma must be positive" % name)
    # oG -> A -> tG, on a 3-D grid oG -> A -> B -> tG: oG is only read, so `oG is tG` needs no copy
    tmp = [s._alloc(kind, zero=False) for _ in range(2 if oG.sz > 1 else 1)]
    try:
        mdim = ctypes.c_int(0)
        lib.call("mf_datagen_blur", oG.sx, oG.sy, oG.sz, ncomp, oG.ptr, tG.ptr, _ptr(tmp[0]), _ptr(tmp[1]) if len(tmp) > 1 else None,
                 float(sigma), ctypes.byref(mdim), s.stream)
    finally:
        for t in reversed(tmp):
            s._release(kind, t)
    return int(mdim.value)


@plugin
def blurMacGrid(oG, tG, si):
    """initplugins.cpp:616-651: the separable Gaussian blur of sigma si (weights not normalised, taps clamped into the grid) of every
    component at the cell's own index; returns the kernel's length.  Stricter than the reference: si <= 0 or not finite is a
    ValueError (the reference fills the grid with NaN)."""
    return _blur("blurMacGrid", MACGrid, "MACGrid", "vec", 3, oG, tG, si)


@plugin
def blurRealGrid(oG, tG, si):
    """initplugins.cpp:602-613, 653-655: the same blur of a Grid<Real>"""
    return _blur("blurRealGrid", Grid, "Grid<Real>", "real", 1, oG, tG, si)


@plugin
def calcCenterOfMass(density):
    """initplugins.cpp:337-348: sum(density * cell centre) / sum(density), undivided where the fp32 sum of density is <= 1e-6.  The
    terms are the reference's fp32 products; the sums are fp64 in a fixed order (the reference's serial fp32 sum has no parallel
    form) and each quotient is rounded once.  One read-back of three floats."""
    s, lib = _datagen_lib("calcCenterOfMass", density)
    _chk(density, Grid, "Grid<Real>")
    out = (ctypes.c_float * 3)()
    lib.call("mf_datagen_center_of_mass", density.sx, density.sy, density.sz, density.ptr, out, s.stream)
    return vec3(float(out[0]), float(out[1]), float(out[2]))


def _project(name, val, shadeMode, scale, views=7):
    s, lib = _datagen_lib(name, val)
    _chk(val, Grid, "Grid<Real>")
    w = val.sx + val.sz + val.sx if val.sz > 1 else val.sx
    h = max(val.sx, val.sy, val.sz)
    img = torch.empty(h * w * 3, dtype=torch.uint8, device=s.device)
    light = s._alloc("real", zero=False) if shadeMode == 1 else None       # the reference's grid L, which only surface mode reads
    try:
        lib.call("mf_datagen_project", val.sx, val.sy, val.sz, val.ptr, _ptr(light), int(shadeMode), float(np.float32(scale)), int(views), _ptr(img),
                 s.stream)
    finally:
        if light is not None:
            s._release("real", light)
    return img.cpu().numpy().reshape(h, w, 3)


@plugin
def projectImage(val, shadeMode=0, scale=1.):
    """what projectPpmFull writes, as the (h, w, 3) uint8 array in file row order (top row first): the view along z and, on a 3-D
    grid, the views along x and y beside it; shadeMode 1 composites lit surfaces, every other value accumulates smoke.  One thread
    per pixel marches in the reference's order, so the bytes are the reference's.  One read-back of the image."""
    return _project("projectImage", val, shadeMode, scale)


@plugin
def projectPpmFull(val, name, shadeMode=0, scale=1.):
    """initplugins.cpp:273-282: projectImage written as a binary .ppm"""
    img = _project("projectPpmFull", val, shadeMode, scale)
    try:
        f = open(name, "wb")
    except OSError as e:
        raise RuntimeError("projectPpmFull: unable to open '%s' for writing (%s)" % (name, e.strerror))
    with f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def _stencil(name, out, grid):
    s, lib = _datagen_lib(name, out, grid)
    _chk(out, Grid, "Grid<Real>"); _chk(grid, Grid, "Grid<Real>")
    out._check_same(grid)
    if out is grid or out.data.data_ptr() == grid.data.data_ptr():
        raise ValueError("%s: the output grid must not be the input grid" % name)
    return s, lib


@plugin
def getLaplacian(laplacian, grid):
    """flip.cpp:779-781, LaplaceOp on the interior; the border of `laplacian` keeps its values.  Stricter than the reference: the
    output may not be the input (the reference's result would depend on its thread schedule)."""
    s, lib = _stencil("getLaplacian", laplacian, grid)
    lib.call("mf_datagen_laplacian", grid.sx, grid.sy, grid.sz, grid.ptr, laplacian.ptr, s.stream)


@plugin
def getCurvature(curv, grid, h=1.0):
    """flip.cpp:783-785, CurvatureOp on the interior: the mean curvature of the level set `grid` with cell size h; the border of
    `curv` keeps its values.  The output may not be the input."""
    s, lib = _stencil("getCurvature", curv, grid)
    lib.call("mf_datagen_curvature", grid.sx, grid.sy, grid.sz, grid.ptr, curv.ptr, float(np.float32(h)), s.stream)


# =========================================================================================================
# obstacle coupling of the moving-obstacle scenes (include/open/manta_hip_movingobs.h)
# =========================================================================================================
@plugin
def set_wall_bcs2(flags, vel, obvel):
    """extforces.cpp:337-373: on every face between a fluid cell and an obstacle cell the normal velocity becomes the obstacle's (obvel
    at the same face); on a 2-D grid vel.z = 0 in every cell"""
    s = flags.parent if isinstance(flags, FlagGrid) else vel.parent
    lib = _extension_lib(s, "set_wall_bcs2", "movingobs")
    _chk(flags, FlagGrid, "FlagGrid"); _chk(vel, MACGrid, "MACGrid"); _chk(obvel, MACGrid, "MACGrid")
    flags._check_same(vel); flags._check_same(obvel)
    lib.call("mf_movingobs_set_wall_bcs2", flags.sx, flags.sy, flags.sz, flags.ptr, vel.ptr, obvel.ptr, s.stream)


@plugin
def resetPhiInObs(flags, sdf):
    """advection.cpp:397-402: sdf = 0.1 in obstacle cells where it is negative, so that the surface does not stick inside obstacles"""
    s = flags.parent if isinstance(flags, FlagGrid) else sdf.parent
    lib = _extension_lib(s, "resetPhiInObs", "movingobs")
    _chk(flags, FlagGrid, "FlagGrid"); _chk(sdf, Grid, "Grid<Real>")
    flags._check_same(sdf)
    lib.call("mf_movingobs_reset_phi_in_obs", flags.n, flags.ptr, sdf.ptr, s.stream)


# =========================================================================================================
# the remaining grid plugins (include/open/manta_hip_gridops.h)
# =========================================================================================================
def _gridops(name, *objs):
    """the solver of the first grid among objs and its library, refused by `name` on a z-slab solver or a backend without the extension
    before any argument is looked at"""
    s = next((o.parent for o in objs if isinstance(o, GridBase)), None)
    if s is None:
        raise RuntimeError("%s: can't convert argument to Grid*" % name)
    return s, _extension_lib(s, name, "gridops")


def _force_field(name, flags, vel, force, region, additive, isMAC):
    s, lib = _gridops(name, flags, vel, force)
    _chk(flags, FlagGrid, "FlagGrid"); _chk(vel, MACGrid, "MACGrid"); _chk(force, VecGrid, "Grid<Vec3>")
    region = _opt(region, Grid, "Grid<Real>")
    flags._check_same(vel); flags._check_same(force)
    if region is not None:
        flags._check_same(region)
    lib.call("mf_gridops_force_field", flags.sx, flags.sy, flags.sz, flags.ptr, vel.ptr, force.ptr, None if region is None else region.ptr,
             additive, int(isMAC), s.stream)


@plugin
def addForceField(flags, vel, force, region=None, isMAC=False):
    """extforces.cpp:430-432 -> KnApplyForceField: vel += the force at the face (force itself with isMAC, else the mean of the two cells)
    on the faces between fluid / fluid and fluid / empty cells of the interior; cells where region > 0 are left out"""
    _force_field("addForceField", flags, vel, force, region, 1, isMAC)


@plugin
def setForceField(flags, vel, force, region=None, isMAC=False):
    """extforces.cpp:434-436 -> KnApplyForceField: like addForceField, but vel = the force at the face"""
    _force_field("setForceField", flags, vel, force, region, 0, isMAC)


@plugin
def setInitialVelocity(flags, vel, invel):
    """extforces.cpp:405-407 -> KnAddForceIfLower: vel + f on the same faces, clamped so that it does not pass the larger (f > 0) or the
    smaller of vel and f"""
    s, lib = _gridops("setInitialVelocity", flags, vel, invel)
    _chk(flags, FlagGrid, "FlagGrid"); _chk(vel, MACGrid, "MACGrid"); _chk(invel, VecGrid, "Grid<Vec3>")
    flags._check_same(vel); flags._check_same(invel)
    lib.call("mf_gridops_add_force_if_lower", flags.sx, flags.sy, flags.sz, flags.ptr, vel.ptr, invel.ptr, s.stream)


@plugin
def extrapolateVec3Simple(vel, phi, distance=4, inside=False):
    """fastmarch.cpp:525-557: cell-centred Vec3 values are carried `distance` layers outwards from the cells with phi < 0 (inside: phi > 0),
    each new cell the per-component mean of its neighbours of the previous layer; every interior cell that is not reached becomes 0"""
    s, lib = _gridops("extrapolateVec3Simple", vel, phi)
    _chk(vel, VecGrid, "Grid<Vec3>"); _chk(phi, Grid, "Grid<Real>")
    vel._check_same(phi)
    tmp = s._alloc("int", zero=False)
    try:
        lib.call("mf_gridops_extrapolate_vec3_simple", vel.sx, vel.sy, vel.sz, vel.ptr, phi.ptr, int(distance), int(inside), _ptr(tmp), s.stream)
    finally:
        s._release("int", tmp)


@plugin
def applyEmission(flags, target, source, emissionTexture=None, isAbsolute=True, type=0):
    """initplugins.cpp:126-128 -> KnApplyEmission: target = source (isAbsolute) or target += source; a cell is skipped only where its
    flag does not match a given type AND the given emissionTexture is 0 there"""
    s, lib = _gridops("applyEmission", flags, target, source)
    _chk(flags, FlagGrid, "FlagGrid"); _chk(target, Grid, "Grid<Real>"); _chk(source, Grid, "Grid<Real>")
    tex = _opt(emissionTexture, Grid, "Grid<Real>")
    for g in (target, source) + (() if tex is None else (tex,)):
        flags._check_same(g)
    lib.call("mf_gridops_apply_emission", flags.n, flags.ptr, target.ptr, source.ptr, None if tex is None else tex.ptr, int(isAbsolute),
             int(type), s.stream)


@plugin
@real_parameters("resetValue")
def resetInObstacle(flags, vel, density, heat=None, fuel=None, flame=None, red=None, green=None, blue=None, resetValue=0):
    """initplugins.cpp:179-183 -> KnResetInObstacle: vel and every given grid = resetValue in the obstacle cells; flame goes with fuel,
    green and blue go with red.  resetValue is a Real whose default the reference spells 0."""
    s, lib = _gridops("resetInObstacle", flags, vel)
    _chk(flags, FlagGrid, "FlagGrid"); _chk(vel, MACGrid, "MACGrid")
    g = [_opt(x, Grid, "Grid<Real>") for x in (density, heat, fuel, flame, red, green, blue)]
    if g[2] is not None and g[3] is None:
        raise RuntimeError("resetInObstacle: fuel is given without flame")
    if g[4] is not None and (g[5] is None or g[6] is None):
        raise RuntimeError("resetInObstacle: red is given without green and blue")
    flags._check_same(vel)
    for x in g:
        if x is not None:
            flags._check_same(x)
    lib.call("mf_gridops_reset_in_obstacle", flags.n, flags.ptr, vel.ptr, *([None if x is None else x.ptr for x in g] +
             [float(np.float32(resetValue)), s.stream]))


@plugin
def copyMACData(source, target, flags, flag, bnd):
    """grid.cpp:1013-1033: target = source in the cells at least bnd from every side whose flags have a bit of `flag`"""
    s, lib = _gridops("copyMACData", source, target, flags)
    _chk(source, MACGrid, "MACGrid"); _chk(target, MACGrid, "MACGrid"); _chk(flags, FlagGrid, "FlagGrid")
    if source.dims != target.dims:
        raise RuntimeError("different grid resolutions [%d,%d,%d] vs [%d,%d,%d]" % (source.dims + target.dims))
    target._check_same(flags)
    if int(bnd) < 0:
        raise RuntimeError("copyMACData: bnd %d is negative: the reference reads outside the grid" % int(bnd))
    lib.call("mf_gridops_copy_mac_data", target.sx, target.sy, target.sz, source.ptr, target.ptr, flags.ptr, int(flag), int(bnd), s.stream)


@plugin
def copyRealToVec3(sourceX, sourceY, sourceZ, target):
    """grid.cpp:527-536: the three Real grids become the components of target"""
    s, lib = _gridops("copyRealToVec3", sourceX, sourceY, sourceZ, target)
    for g in (sourceX, sourceY, sourceZ):
        _chk(g, Grid, "Grid<Real>")
    _chk(target, VecGrid, "Grid<Vec3>")
    for g in (sourceX, sourceY, sourceZ):
        target._check_same(g)
    n = target.n
    lib.call("mf_gridops_copy_planes", n, sourceX.ptr, sourceY.ptr, sourceZ.ptr, target.ptr, _ptr(target.data[n:]), _ptr(target.data[2 * n:]),
             s.stream)


@plugin
def copyVec3ToReal(source, targetX, targetY, targetZ):
    """grid.cpp:516-525: the components of source go to the three Real grids"""
    s, lib = _gridops("copyVec3ToReal", source, targetX, targetY, targetZ)
    _chk(source, VecGrid, "Grid<Vec3>")
    for g in (targetX, targetY, targetZ):
        _chk(g, Grid, "Grid<Real>")
        source._check_same(g)
    n = source.n
    lib.call("mf_gridops_copy_planes", n, source.ptr, _ptr(source.data[n:]), _ptr(source.data[2 * n:]), targetX.ptr, targetY.ptr, targetZ.ptr,
             s.stream)


@plugin
def resampleMacToVec3(source, target):
    """grid.cpp:496-505: target = source.getCentered(i, j, k) on the interior; the border of target keeps its values"""
    s, lib = _gridops("resampleMacToVec3", source, target)
    _chk(source, MACGrid, "MACGrid"); _chk(target, VecGrid, "Grid<Vec3>")
    source._check_same(target)
    if source.data.data_ptr() == target.data.data_ptr():
        raise RuntimeError("resampleMacToVec3: target must not be source")
    lib.call("mf_gridops_resample_mac_to_vec3", source.sx, source.sy, source.sz, source.ptr, target.ptr, s.stream)


@plugin
def swapComponents(vel, c1=0, c2=1, c3=2):
    """grid.cpp:564-571: (x, y, z) = (v[c1], v[c2], v[c3]) of the old value in every cell"""
    s, lib = _gridops("swapComponents", vel)
    _chk(vel, VecGrid, "Grid<Vec3>")
    if not all(0 <= c <= 2 for c in (c1, c2, c3)):
        raise RuntimeError("swapComponents: component (%d, %d, %d) outside 0..2: the reference reads outside the vector" % (c1, c2, c3))
    lib.call("mf_gridops_swap_components", vel.n, vel.ptr, c1, c2, c3, s.stream)


@plugin
def getGridAvg(source, flags=None):
    """grid.cpp:728-739: the mean of source over every cell, or over the fluid cells of flags; an fp64 sum (the device's fixed-order
    reduction) times 1 / count, as fp32; -1 where there is no such cell"""
    s, lib = _gridops("getGridAvg", source, flags)
    _chk(source, Grid, "Grid<Real>")
    flags = _opt(flags, FlagGrid, "FlagGrid")
    if flags is not None:
        source._check_same(flags)
    r = ctypes.c_float()
    lib.call("mf_gridops_grid_avg", source.n, source.ptr, None if flags is None else flags.ptr, ctypes.byref(r), s.stream)
    return r.value


def _simple_noise(name, is_vec, flags, target, noise, scale, weight):
    s, lib = _gridops(name, flags, target)
    _chk(flags, FlagGrid, "FlagGrid")
    _chk(target, VecGrid, "Grid<Vec3>") if is_vec else _chk(target, Grid, "Grid<Real>")
    if not hasattr(noise, "_tile") or not hasattr(noise, "_params"):
        raise RuntimeError("can't convert argument to WaveletNoiseField*")
    weight = _opt(weight, Grid, "Grid<Real>")
    flags._check_same(target)
    if weight is not None:
        flags._check_same(weight)
    lib.call("mf_gridops_simple_noise", int(is_vec), flags.sx, flags.sy, flags.sz, flags.ptr, target.ptr, _ptr(noise._tile), noise._params(),
             float(np.float32(scale)), None if weight is None else weight.ptr, s.stream)


@plugin
def applySimpleNoiseVec3(flags, target, noise, scale=1.0, weight=None):
    """waveletturbulence.cpp:94-99 -> knApplySimpleNoiseVec3: target += noise.evaluateCurl(cell centre) * scale * weight on fluid cells; no
    position scaling, no uv grid"""
    _simple_noise("applySimpleNoiseVec3", True, flags, target, noise, scale, weight)


@plugin
def applySimpleNoiseReal(flags, target, noise, scale=1.0, weight=None):
    """waveletturbulence.cpp:112-116 -> knApplySimpleNoiseReal: target += noise.evaluate(cell centre) * scale * weight on fluid cells"""
    _simple_noise("applySimpleNoiseReal", False, flags, target, noise, scale, weight)


def _legacy_potential(name, which, pot, flags, v, radius, normal, tauMin, tauMax, scaleFromManta, itype, jtype):
    s, lib = _gridops(name, pot, flags, v)
    _chk(pot, Grid, "Grid<Real>"); _chk(flags, FlagGrid, "FlagGrid"); _chk(v, MACGrid, "MACGrid")
    if which == 1:
        _chk(normal, VecGrid, "Grid<Vec3>")
        pot._check_same(normal)
    pot._check_same(flags); pot._check_same(v)
    if not 0 <= int(radius) <= 16:
        raise RuntimeError("%s: radius %d outside 0..16" % (name, int(radius)))
    lib.call("mf_gridops_legacy_potential", which, pot.sx, pot.sy, pot.sz, pot.ptr, flags.ptr, v.ptr, None if normal is None else normal.ptr,
             int(radius), float(np.float32(tauMin)), float(np.float32(tauMax)), float(np.float32(scaleFromManta)), int(itype), int(jtype), s.stream)


@plugin
def flipComputePotentialTrappedAir(pot, flags, v, radius, tauMin, tauMax, scaleFromManta, itype=1, jtype=1):
    """secondaryparticles.cpp:579-587 (legacy; flipComputeSecondaryParticlePotentials is the combined form): the trapped-air potential
    of the interior cells with flags & itype from their neighbours with flags & jtype; pot is cleared first.  Every itype cell must be
    `radius` cells from each side and no neighbour may lie on the upper outermost layer: the reference reads outside the grid otherwise,
    and here such a neighbour is skipped where its words leave the array."""
    _legacy_potential("flipComputePotentialTrappedAir", 0, pot, flags, v, radius, None, tauMin, tauMax, scaleFromManta, itype, jtype)


@plugin
def flipComputePotentialKineticEnergy(pot, flags, v, tauMin, tauMax, scaleFromManta, itype=1):
    """secondaryparticles.cpp:604-611 (legacy): 0.5 * 125 * |v|^2 of every cell with flags & itype, clamped between the thresholds"""
    _legacy_potential("flipComputePotentialKineticEnergy", 2, pot, flags, v, 0, None, tauMin, tauMax, scaleFromManta, itype, 0)


@plugin
def flipComputePotentialWaveCrest(pot, flags, v, radius, normal, tauMin, tauMax, scaleFromManta, itype=1, jtype=1):
    """secondaryparticles.cpp:650-658 (legacy): the wave-crest potential from the surface normals of flipComputeSurfaceNormals; the same
    preconditions as flipComputePotentialTrappedAir"""
    _legacy_potential("flipComputePotentialWaveCrest", 1, pot, flags, v, radius, normal, tauMin, tauMax, scaleFromManta, itype, jtype)


@plugin
def flipComputeSurfaceNormals(normal, phi):
    """secondaryparticles.cpp:666-670 (legacy): normal = the central-difference gradient of phi on the interior, then normalised in
    every cell (the border's own values included)"""
    s, lib = _gridops("flipComputeSurfaceNormals", normal, phi)
    _chk(normal, VecGrid, "Grid<Vec3>"); _chk(phi, Grid, "Grid<Real>")
    normal._check_same(phi)
    lib.call("mf_gridops_surface_normals", normal.sx, normal.sy, normal.sz, normal.ptr, phi.ptr, s.stream)


@plugin
def flipUpdateNeighborRatio(flags, neighborRatio, radius, itype=1, jtype=2):
    """secondaryparticles.cpp:699-706 (legacy): the itype neighbours within radius over the neighbours that are not jtype (jtype means
    "skip" here, default obstacle); NaN where there is no countable neighbour.  Every itype cell must be `radius` cells from each side."""
    s, lib = _gridops("flipUpdateNeighborRatio", flags, neighborRatio)
    _chk(flags, FlagGrid, "FlagGrid"); _chk(neighborRatio, Grid, "Grid<Real>")
    flags._check_same(neighborRatio)
    if not 0 <= int(radius) <= 16:
        raise RuntimeError("flipUpdateNeighborRatio: radius %d outside 0..16" % int(radius))
    lib.call("mf_gridops_neighbor_ratio", flags.sx, flags.sy, flags.sz, flags.ptr, neighborRatio.ptr, int(radius), int(itype), int(jtype), s.stream)


@plugin
def debugIntToReal(source, dest, factor=1.):
    """flip.cpp:266-269: dest = Real(source) * factor"""
    s, lib = _gridops("debugIntToReal", source, dest)
    _chk(source, core.IntGrid, "Grid<int>"); _chk(dest, Grid, "Grid<Real>")
    source._check_same(dest)
    lib.call("mf_gridops_int_to_real", source.n, source.ptr, dest.ptr, float(np.float32(factor)), s.stream)
