"""Surface turbulence (plugin/surfaceturbulence.cpp; Mercier et al., "Surface Turbulence for Particle-Based Liquid Simulations") on
include/open/manta_hip_surfturb.h.  DESIGN.md section 27 has the contract.

This module is opt-in: ``mantaflow_amd.api`` does not import it, so ``from manta import *`` does not have the names.  A scene gets
them with ``from mantaflow_amd.surfturb import *`` in front of ``from manta import *``.

The reference keeps frameCount, both acceleration grids and their resolutions in process-wide globals, so one process holds one
surface simulation; ``resetSurfaceTurbulenceState`` puts that state back to a fresh process's.  The host orchestrates the stages and
reads back scalars only: per maintenance iteration the number of buffered points, the kill counts and one flag per greedy round.
"""
import ctypes

import torch

from .core import BasicParticleSystem, FlagGrid, PdataReal, PdataVec3, _extension_lib, _ptr
from .plugins import plugin, real_parameters

__all__ = ["particleSurfaceTurbulence", "debugCheckParts", "resetSurfaceTurbulenceState", "lastSurfaceTurbulenceStats"]

_WHAT = "particleSurfaceTurbulence"


class _State(object):
    """the reference's globals (:277-282): frameCount and the resolutions of accelCoarse / accelSurface, fixed by the first call"""

    def __init__(self):
        self.frameCount, self.Rc, self.Rs = 0, None, None


_state = _State()
_stats = {}


def resetSurfaceTurbulenceState():
    """frameCount back to 0 and the two cell-list resolutions forgotten, as a fresh process of the reference has them (no reference
    counterpart)"""
    global _state
    _state = _State()
    _stats.clear()


def lastSurfaceTurbulenceStats():
    """of the last particleSurfaceTurbulence call: frame, the list resolutions, the size after initFines (first frame), and per
    maintenance iteration the points added, the kill calls of the three delete passes, the rounds of the greedy pass, whether the
    iteration compressed and the size it left; `compressions` counts the latter"""
    return {k: (list(v) if isinstance(v, list) else v) for k, v in _stats.items()}


def _al(n):
    return (int(n) + 255) & ~255


class _Run(object):
    """one call's view of the arrays: the parameter block, the two cell lists, and the scratch block cut into its slices.  The stages
    are methods, so the tests drive them one at a time."""

    def __init__(self, lib, s, flags, coarse, prev, surf, chan, par, Rc, Rs):
        self.lib, self.s, self.flags, self.coarse, self.prev, self.surf, self.chan = lib, s, flags, coarse, prev, surf, chan
        self.par, self.Rc, self.Rs = par, int(Rc), int(Rs)
        self._block, self._release, self._cap = None, None, -1
        # the lists outlive a growth of the point arrays: the starts and the coarse ids are cut once, the surface ids are carried over
        nc = max(coarse.np, 1)
        self._fixed, self._release_fixed = self._take(_al(4 * (self.Rc ** 3 + 1)) + _al(4 * nc) + _al(4 * (self.Rs ** 3 + 1)) + 256)
        p = (self._fixed.data_ptr() + 255) & ~255
        self.lists = {}
        for name, b in (("cstart", 4 * (self.Rc ** 3 + 1)), ("cids", 4 * nc), ("sstart", 4 * (self.Rs ** 3 + 1))):
            self.lists[name] = ctypes.c_void_p(p)
            p += _al(b)
        self._sids = torch.empty(max(surf.cap, 1), dtype=torch.int32, device=s.device)
        self.ensure()

    # ---- scratch: cell starts and ids of both lists, one Vec3 and one Real per surface point, the add pass's candidates and
    # marks, the greedy pass's two states, the head and the sort / scan workspace; from the solver's pool where a grid is large enough
    def _take(self, nbytes):
        s = self.s
        for kind, size in (("int", 4 * s.ncells), ("vec", 12 * s.ncells)):
            if nbytes <= size:
                t = s._alloc(kind, zero=False)
                return t, (lambda: s._release(kind, t))
        return torch.empty(nbytes, dtype=torch.uint8, device=s.device), (lambda: None)

    def ensure(self):
        cap, nc = max(self.surf.cap, 1), max(self.coarse.np, 1)
        if cap == self._cap:
            return
        self.release()
        need = ctypes.c_int64(0)
        self.lib.call("mf_surfturb_tmp_bytes", max(cap, nc), max(self.Rc, self.Rs) ** 3, cap, ctypes.byref(need))
        if self._sids.numel() < cap:
            grown = torch.empty(cap, dtype=torch.int32, device=self.s.device)
            grown[:self._sids.numel()] = self._sids
            self._sids = grown
        sizes = [("head", 256), ("tempv", 12 * cap), ("tempf", 4 * cap), ("cand", 12 * cap), ("mark", 4 * cap), ("st0", 4 * cap), ("st1", 4 * cap),
                 ("tmp", need.value)]
        total = sum(_al(b) for _, b in sizes) + 256
        self._block, self._release = self._take(total)
        p = (self._block.data_ptr() + 255) & ~255
        self.off = {}
        for name, b in sizes:
            self.off[name] = ctypes.c_void_p(p)
            p += _al(b)
        self.off.update(self.lists, sids=_ptr(self._sids))
        self.tmp_bytes, self._cap = int(need.value), cap

    def release(self):
        if self._release is not None:
            self._release()
        self._block, self._release, self._cap = None, None, -1

    def close(self):
        self.release()
        if self._release_fixed is not None:
            self._release_fixed()
        self._release_fixed = None

    # ---- argument groups
    def _c(self):
        c = self.coarse
        return (self.Rc, self.off["cstart"], self.off["cids"], c.np, c.cap, _ptr(c.pos), _ptr(c.flag))

    def _sl(self):
        return (self.Rs, self.off["sstart"], self.off["sids"])

    def _call(self, name, *a):
        self.lib.call(name, *(a + (self.s.stream,)))

    # ---- the stages
    def coarse_list(self, of_prev=False):
        c = self.coarse
        src, cap = (self.prev.data, self.prev.cap) if of_prev else (c.pos, c.cap)
        self._call("mf_surfturb_cells", self.par, self.Rc, c.np, cap, _ptr(src), self.off["cstart"], self.off["cids"], self.off["tmp"], self.tmp_bytes)

    def surface_list(self, empty=False):
        sp = self.surf
        self._call("mf_surfturb_cells", self.par, self.Rs, 0 if empty else sp.np, sp.cap, _ptr(sp.pos), self.off["sstart"], self.off["sids"],
                   self.off["tmp"], self.tmp_bytes)

    def init_fines(self):
        lib, s, c, sp = self.lib, self.s, self.coarse, self.surf
        count = ctypes.c_int64(0)
        lib.call("mf_surfturb_directions", self.par, 0, None, ctypes.byref(count))
        nd = int(count.value)
        host = (ctypes.c_float * (3 * max(nd, 1)))()
        lib.call("mf_surfturb_directions", self.par, nd, host, ctypes.byref(count))
        dirs = torch.tensor(list(host), dtype=torch.float32, device=s.device)
        m = c.np * nd
        mark = torch.empty(max(m, 1), dtype=torch.int32, device=s.device)
        need = ctypes.c_int64(0)
        lib.call("mf_surfturb_tmp_bytes", 0, 1, max(m, 1), ctypes.byref(need))
        tmp = torch.empty(int(need.value), dtype=torch.uint8, device=s.device)
        total = ctypes.c_int64(0)
        g = self.flags
        self._call("mf_surfturb_init_plan", self.par, g.sx, g.sy, g.sz, g.ptr, *(self._c() + (nd, _ptr(dirs), _ptr(mark), _ptr(tmp), int(need.value),
                   ctypes.byref(total))))
        total = int(total.value)
        sp.clear()                      # surfacePoints.clear(), then addParticle per point: zero channels, mDeleteChunk = size / 20
        sp.resizeAll(total)
        if total:
            sp.mDeleteChunk = total // 20
        self.ensure()
        self._call("mf_surfturb_init_fill", self.par, c.np, c.cap, _ptr(c.pos), nd, _ptr(dirs), _ptr(mark), sp.cap, _ptr(sp.pos), _ptr(sp.flag))
        return total

    def advect(self):
        c, sp = self.coarse, self.surf
        self._call("mf_surfturb_advect", self.par, self.Rc, self.off["cstart"], self.off["cids"], c.np, c.cap, _ptr(c.pos), _ptr(c.flag),
                   self.prev.cap, _ptr(self.prev.data), sp.np, sp.cap, _ptr(sp.pos), _ptr(sp.flag))

    def add(self):
        """the add pass, the first doCompress and insertBufferedParticles; -> points added"""
        sp = self.surf
        n = sp.np
        if sp.mDeletes > sp.mDeleteChunk:
            # the first doCompress never compresses while the system is only touched by this plugin
            raise RuntimeError("%s: the surface points carry %d uncompressed deletes beyond their chunk of %d -- call doCompress() before the plugin"
                               % (_WHAT, sp.mDeletes, sp.mDeleteChunk))
        if sp.cap < 2 * n:              # at most n points are buffered: grow before the plan, so its slices of the scratch stay where they are
            sp.reserve(2 * n)
            self.ensure()
        total = ctypes.c_int64(0)
        self._call("mf_surfturb_add_plan", self.par, *(self._c() + self._sl() + (n, sp.cap, _ptr(sp.pos), _ptr(sp.flag), self.off["cand"], self.off["mark"],
                   self.off["tmp"], self.tmp_bytes, ctypes.byref(total))))
        total = int(total.value)
        if n == 0:
            return 0
        if total:
            pc, pm = self.off["cand"], self.off["mark"]
            sp.resizeAll(n + total, sp.cap)
            self._call("mf_surfturb_add_apply", n, total, sp.cap, _ptr(sp.pos), _ptr(sp.flag), pc, pm)
            for pd in sp.pdata:         # new points get zero entries in every channel
                for k in range(pd._ncomp):
                    pd.data[k * pd.cap + n:k * pd.cap + n + total] = 0
        else:
            self._call("mf_surfturb_clear_new", n, _ptr(sp.flag))
        return total

    def delete(self):
        """the three delete passes; -> (rounds of the greedy pass, kill calls per pass)"""
        sp = self.surf
        n = sp.np
        if n == 0:
            return 0, (0, 0, 0)
        a, b = self.off["st0"], self.off["st1"]
        rounds, undecided = 0, ctypes.c_int32(1)
        while undecided.value:
            if rounds > n:
                raise RuntimeError("%s: the greedy delete pass did not end within %d rounds" % (_WHAT, n))
            self._call("mf_surfturb_greedy_round", self.par, *(self._sl() + (n, sp.cap, _ptr(sp.pos), _ptr(sp.flag), int(rounds == 0), a, b, self.off["head"],
                       ctypes.byref(undecided))))
            a, b = b, a
            rounds += 1
        kills = (ctypes.c_int32 * 3)()
        self._call("mf_surfturb_delete", self.par, *(self._c() + (n, sp.cap, _ptr(sp.pos), _ptr(sp.flag), a, self.off["head"], kills)))
        kills = tuple(int(k) for k in kills)
        sp.mDeletes += sum(kills)
        return rounds, kills

    def compress_and_insert(self):
        """the second doCompress and insertBufferedParticles (nothing is buffered: PNEW is cleared everywhere); -> compressed?"""
        sp = self.surf
        did = sp.mDeletes > sp.mDeleteChunk
        if did:
            sp.compress()
        self._call("mf_surfturb_clear_new", sp.np, _ptr(sp.flag))
        return did

    def normals(self):
        sp = self.surf
        self._call("mf_surfturb_normals", self.par, *(self._c() + self._sl() + (sp.np, sp.cap, _ptr(sp.pos), _ptr(sp.flag), _ptr(self.chan["normals"].data),
                   self.off["tempv"])))

    def regularize(self):
        sp = self.surf
        self._call("mf_surfturb_regularize", self.par, *(self._sl() + (sp.np, sp.cap, _ptr(sp.pos), _ptr(sp.flag), _ptr(self.chan["normals"].data),
                   self.off["tempf"], self.off["tempv"])))

    def constrain(self):
        sp = self.surf
        self._call("mf_surfturb_constrain", self.par, *(self._c() + (sp.np, sp.cap, _ptr(sp.pos))))

    def waves(self):
        sp, ch = self.surf, self.chan
        self._call("mf_surfturb_waves", self.par, *(self._sl() + (sp.np, sp.cap, _ptr(sp.pos), _ptr(sp.flag), _ptr(ch["normals"].data), _ptr(ch["H"].data),
                   _ptr(ch["DtH"].data), _ptr(ch["source"].data), _ptr(ch["seed"].data), _ptr(ch["seedAmp"].data), self.off["tempf"], self.off["tempv"])))

    def maintenance_iteration(self):
        """one pass of surfaceMaintenance's loop (:785-799; interpolateNewWaveData is dead in the reference and not built); -> stats"""
        added = self.add()
        rounds, kills = self.delete()
        compressed = self.compress_and_insert()
        self.surface_list()
        self.normals()
        self.regularize()
        self.surface_list()
        self.constrain()
        self.surface_list()
        return dict(added=added, rounds=rounds, kills=kills, compressed=compressed, size=self.surf.np)

    def save_prev(self):
        c = self.coarse
        self._call("mf_surfturb_save_prev", c.np, c.cap, _ptr(c.pos), _ptr(c.flag), self.prev.cap, _ptr(self.prev.data))

    def displaced(self, out):
        sp = self.surf
        total = ctypes.c_int64(0)
        self._call("mf_surfturb_displaced_plan", sp.np, _ptr(sp.flag), self.off["mark"], self.off["tmp"], self.tmp_bytes, ctypes.byref(total))
        total = int(total.value)
        out.clear()
        out.resizeAll(total)
        if total:
            out.mDeleteChunk = total // 20
        self._call("mf_surfturb_displaced_fill", sp.np, sp.cap, _ptr(sp.pos), _ptr(sp.flag), _ptr(self.chan["normals"].data), _ptr(self.chan["H"].data),
                   self.off["mark"], max(out.cap, 1), _ptr(out.pos), _ptr(out.flag))
        return total


def _params(lib, frameCount, res, outerRadius, surfaceDensity, dt, waveSpeed, waveDamping, waveSeedFrequency, waveMaxAmplitude, waveMaxFrequency,
            waveMaxSeedingAmplitude, center, radius, step):
    """-> (the parameter block, (Rc, Rs) of these parameters); host code of the library"""
    par, rr = (ctypes.c_float * 32)(), (ctypes.c_int32 * 2)()
    lib.call("mf_surfturb_params", int(res), float(outerRadius), int(surfaceDensity), float(dt), float(waveSpeed), float(waveDamping),
             float(waveSeedFrequency), float(waveMaxAmplitude), float(waveMaxFrequency), float(waveMaxSeedingAmplitude), float(center), float(radius),
             float(step), int(frameCount), par, rr)
    return par, (int(rr[0]), int(rr[1]))


def _channel(pd, cls, what, system):
    if not isinstance(pd, cls):
        raise RuntimeError("can't convert argument to %s*" % what)
    if pd.sys is not system:
        raise RuntimeError("%s: a channel is not registered with its particle system" % _WHAT)
    return pd


@plugin
@real_parameters("waveSeedFrequency", "waveMaxFrequency")
def particleSurfaceTurbulence(flags, coarseParts, coarsePartsPrevPos, surfPoints, surfaceNormals, surfaceWaveH, surfaceWaveDtH, surfacePointsDisplaced,
                              surfaceWaveSource, surfaceWaveSeed, surfaceWaveSeedAmplitude, res, outerRadius=1.0, surfaceDensity=20,
                              nbSurfaceMaintenanceIterations=4, dt=0.005, waveSpeed=16.0, waveDamping=0.0, waveSeedFrequency=4, waveMaxAmplitude=0.25,
                              waveMaxFrequency=800, waveMaxSeedingAmplitude=0.5, waveSeedingCurvatureThresholdRegionCenter=0.025,
                              waveSeedingCurvatureThresholdRegionRadius=0.01, waveSeedStepSizeRatioOfMax=0.05):
    """surfaceturbulence.cpp:1028-1159.  The first call of a process (see resetSurfaceTurbulenceState) creates the surface points around
    the coarse particles near the surface and runs 6 * nb maintenance iterations; every later call advects the points with the
    coarse particles, runs nb iterations and steps the surface waves.  One device, whole-domain 3-D solvers."""
    if not isinstance(flags, FlagGrid):
        raise RuntimeError("can't convert argument to FlagGrid*")
    s = flags.parent
    lib = _extension_lib(s, _WHAT, "surfturb")
    if s.is2D():
        raise RuntimeError("%s: surface turbulence does not run on a 2-D solver" % _WHAT)
    for p in (coarseParts, surfPoints, surfacePointsDisplaced):
        if not isinstance(p, BasicParticleSystem):
            raise RuntimeError("can't convert argument to BasicParticleSystem*")
    prev = _channel(coarsePartsPrevPos, PdataVec3, "ParticleDataImpl<Vec3>", coarseParts)
    chan = dict(normals=_channel(surfaceNormals, PdataVec3, "ParticleDataImpl<Vec3>", surfPoints))
    for key, pd in (("H", surfaceWaveH), ("DtH", surfaceWaveDtH), ("source", surfaceWaveSource), ("seed", surfaceWaveSeed),
                    ("seedAmp", surfaceWaveSeedAmplitude)):
        chan[key] = _channel(pd, PdataReal, "ParticleDataImpl<Real>", surfPoints)
    st = _state
    par, rr = _params(lib, st.frameCount, res, outerRadius, surfaceDensity, dt, waveSpeed, waveDamping, waveSeedFrequency, waveMaxAmplitude,
                      waveMaxFrequency, waveMaxSeedingAmplitude, waveSeedingCurvatureThresholdRegionCenter, waveSeedingCurvatureThresholdRegionRadius,
                      waveSeedStepSizeRatioOfMax)
    first = st.frameCount == 0
    if first:
        st.Rc, st.Rs = rr
    nb = int(nbSurfaceMaintenanceIterations)
    run = _Run(lib, s, flags, coarseParts, prev, surfPoints, chan, par, st.Rc, st.Rs)
    _stats.clear()
    _stats.update(frame=st.frameCount, Rc=st.Rc, Rs=st.Rs, iterations=[], compressions=0)
    try:
        if first:
            run.coarse_list()
            _stats["init"] = run.init_fines()
            run.surface_list(empty=True)        # nothing fills accelSurface after initFines: the list is empty in the first add / delete
            count = 6 * nb
        else:
            run.coarse_list(of_prev=True)
            run.advect()
            run.surface_list()
            run.coarse_list()
            count = nb
        for _ in range(max(count, 0)):
            it = run.maintenance_iteration()
            _stats["iterations"].append(it)
            _stats["compressions"] += int(it["compressed"])
        if first:
            n = surfPoints.np
            for key in ("H", "DtH", "seed", "seedAmp"):
                chan[key].data[:n] = 0
        else:
            run.waves()
        st.frameCount += 1
        run.save_prev()
        _stats["displaced"] = run.displaced(surfacePointsDisplaced)
        _stats["size"] = surfPoints.np
    finally:
        run.close()


@plugin
def debugCheckParts(parts, flags):
    """surfaceturbulence.cpp:1164-1171 as one reduction; raises where the reference prints and calls exit(1)"""
    if not isinstance(flags, FlagGrid):
        raise RuntimeError("can't convert argument to FlagGrid*")
    s = flags.parent
    lib = _extension_lib(s, "debugCheckParts", "surfturb")
    if not isinstance(parts, BasicParticleSystem):
        raise RuntimeError("can't convert argument to BasicParticleSystem*")
    if parts.np == 0:
        return
    head = torch.empty(64, dtype=torch.int32, device=s.device)
    bad = ctypes.c_int64(-1)
    lib.call("mf_surfturb_check_parts", flags.sx, flags.sy, flags.sz, parts.np, parts.cap, _ptr(parts.pos), _ptr(head), ctypes.byref(bad), s.stream)
    if bad.value >= 0:
        p = parts.getPos(bad.value)
        raise RuntimeError("bad position??? %d [%+4.2f,%+4.2f,%+4.2f]" % (bad.value, p.x, p.y, p.z))
