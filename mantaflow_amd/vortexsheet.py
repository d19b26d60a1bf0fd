"""Vortex sheets (source/vortexsheet.{h,cpp} and the sheet plugins of source/plugin/vortexplugins.cpp) on
include/open/manta_hip_vsheet.h.  DESIGN.md section 28 has the contract.

This module is opt-in: ``mantaflow_amd.api`` does not import it, so ``from manta import *`` does not have the names.  A scene gets
them with ``from mantaflow_amd.vortexsheet import *`` in front of ``from manta import *`` and creates the sheet with
``s.create(VortexSheetMesh)``.

A VortexSheetMesh is a core.Mesh with the reference's fixed channels as structure-of-arrays device planes of the mesh's own strides:
per triangle vorticity, vorticitySmoothed, circulation ([3][tcap]), smokeAmount, smokeParticles ([tcap]); per node tex1, tex2
([3][ncap]) and the turbulence pair k, epsilon ([2][ncap]).  One device, whole-domain 3-D solvers.  Not built:
VortexSheetMesh.calcCirculation (README, "The vortex-sheet mesh and its per-triangle plugins").

texcoordInflow keeps its offset in a process-wide static, as the reference does; ``resetVortexSheetState`` puts it back to zero.
"""
import ctypes

import numpy as np
import torch

from .core import FlagGrid, Grid, MACGrid, Mesh, VecGrid, _extension_lib, _ptr, _to_vec3
from .plugins import plugin, real_parameters

__all__ = ["VortexSheetMesh", "VICintegration", "smoothVorticity", "vorticitySource", "texcoordInflow", "meshSmokeInflow", "resetVortexSheetState",
           "lastVortexSheetStats"]

f32 = np.float32
_TRI_CHANNELS = (("vorticity", 3, 0.0), ("vorticitySmoothed", 3, 0.0), ("circulation", 3, 0.0), ("smokeAmount", 1, 1.0), ("smokeParticles", 1, 0.0))
_NODE_CHANNELS = (("tex1", 3, 0.0), ("tex2", 3, 0.0), ("turb", 2, 0.0))


class _State(object):
    """texcoordInflow's `static Vec3 t0` (vortexplugins.cpp:43)"""

    def __init__(self):
        self.t0 = (0.0, 0.0, 0.0)


_state = _State()
_stats = {}


def resetVortexSheetState():
    """texcoordInflow's static offset back to zero, as a fresh process of the reference has it (no reference counterpart)"""
    global _state
    _state = _State()
    _stats.clear()


def lastVortexSheetStats():
    """`source`: the max and the mean of |vorticity| after the last vorticitySource (what vortexplugins.cpp:119 prints; the mean is an
    fp64 device sum over the triangle count, the reference's a serial fp32 sum); `vic`: per component of the last VICintegration the CG
    iterations and the final residual (what :288 prints)"""
    return {k: (dict(v) if isinstance(v, dict) else [dict(c) for c in v]) for k, v in _stats.items()}


def _sheet_lib(s, name):
    """the library if `name` can run: a z-slab solver, then a backend without the extension, then a 2-D solver are refused by name,
    before any argument is looked at"""
    lib = _extension_lib(s, name, "vsheet")
    if not s.is3D():
        raise RuntimeError("%s: 3-D solvers only" % name)
    return lib


def _real(v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise RuntimeError("argument is not a float")
    return float(f32(v))


def _shape_record(name, shape):
    if not (hasattr(shape, "_inside") and hasattr(shape, "_shape_params")):
        raise RuntimeError("can't convert argument to Shape*")
    kind, q = shape._shape_params()
    if kind is None:
        raise RuntimeError("%s: the library has no isInside of this shape" % name)
    return kind, (ctypes.c_float * 12)(*[float(f32(v)) for v in q])


class VortexSheetMesh(Mesh):
    """VortexSheetMesh, vortexsheet.h:60-84.  Every route that rebuilds the mesh (set_numpy, load, clear, LevelsetGrid.createMesh into
    it) leaves every channel entry at the reference's defaults -- the T() of rebuildChannels() after clear().  A route that
    changes the triangle or node count without knowing the channels (killSmallComponents) leaves them at their old length, and every
    sheet call then refuses the mesh.  save / load are Mesh's: geometry only."""
    _cname_py, _cname_cpp, _T = "VortexSheetMesh", "VortexSheetMesh", ""

    def __init__(self, parent, name="", **kw):
        Mesh.__init__(self, parent, name, **kw)
        self.mTexOffset = (0.0, 0.0, 0.0)
        self._ch = {}
        self._ch_nt = self._ch_nn = 0          # the lengths the channels are of
        self._ch_tcap = self._ch_ncap = -1     # the strides they were laid out with
        self._ch_fresh = True                  # the mesh was rebuilt: the channels take its lengths, at the defaults, on their next use

    # --- the rebuilding routes ---
    def clear(self):
        Mesh.clear(self)
        self._ch_fresh = True

    def set_numpy(self, pos, normal=None, flags=None, tris=None, triFlags=None):
        Mesh.set_numpy(self, pos, normal, flags, tris, triFlags)
        self._ch_fresh = True

    def _layout(self):
        """the channels as defaults of the mesh's lengths and strides"""
        dev = self.parent.device
        for table, cap, n in ((_TRI_CHANNELS, self.tcap, self.nt), (_NODE_CHANNELS, self.ncap, self.nn)):
            for key, ncomp, default in table:
                t = self._ch.get(key)
                if t is None or t.numel() != ncomp * cap:
                    t = self._ch[key] = torch.empty(ncomp * cap, dtype=torch.float32, device=dev)
                if cap:
                    t.view(ncomp, cap)[:, :n] = default
        self._ch_nt, self._ch_nn, self._ch_tcap, self._ch_ncap, self._ch_fresh = self.nt, self.nn, self.tcap, self.ncap, False

    def _channels(self, who):
        """the channel planes, after the length check every sheet call makes before it touches anything"""
        if self._ch_fresh:
            self._layout()
        if (self._ch_nt, self._ch_nn, self._ch_tcap, self._ch_ncap) != (self.nt, self.nn, self.tcap, self.ncap):
            raise RuntimeError("VortexSheetMesh::%s: channels do not match the mesh (%d triangles and %d nodes, channels of %d and %d)"
                               % (who, self.nt, self.nn, self._ch_nt, self._ch_nn))
        return self._ch

    def _lib(self, who):
        return _sheet_lib(self.parent, "VortexSheetMesh::" + who)

    def _mesh_args(self):
        return (self.nt, self.tcap, _ptr(self.tri), self.nn, self.ncap, _ptr(self.pos))

    # --- array access ---
    def _get(self, key, ncomp, cap, n):
        t = self._ch[key].view(ncomp, cap)[:, :n].detach().cpu().numpy()
        return np.ascontiguousarray(t.T) if ncomp > 1 else t[0].copy()

    def sheet_numpy(self):
        """-> dict of vorticity[t][3], vorticitySmoothed[t][3], circulation[t][3], smokeAmount[t], smokeParticles[t]"""
        self._lib("sheet_numpy")
        self._channels("sheet_numpy")
        self.parent.sync()
        return {key: self._get(key, ncomp, self.tcap, self.nt) for key, ncomp, _ in _TRI_CHANNELS}

    def set_sheet_numpy(self, vorticity=None, vorticitySmoothed=None, circulation=None, smokeAmount=None, smokeParticles=None):
        """any subset of the per-triangle channels from host arrays of the mesh's triangle count"""
        self._lib("set_sheet_numpy")
        self._channels("set_sheet_numpy")
        given = dict(vorticity=vorticity, vorticitySmoothed=vorticitySmoothed, circulation=circulation, smokeAmount=smokeAmount,
                     smokeParticles=smokeParticles)
        arrays = {}
        for key, ncomp, _ in _TRI_CHANNELS:
            if given[key] is not None:
                a = np.asarray(given[key], f32).reshape(-1, ncomp)
                if a.shape[0] != self.nt:
                    raise RuntimeError("VortexSheetMesh::set_sheet_numpy: %s has %d entries, the mesh %d triangles" % (key, a.shape[0], self.nt))
                arrays[key] = (a, ncomp)
        for key, (a, ncomp) in arrays.items():
            if self.nt:
                self._ch[key].view(ncomp, self.tcap)[:, :self.nt] = torch.from_numpy(np.ascontiguousarray(a.T)).to(self.parent.device)

    def tex_numpy(self):
        """-> tex1[n][3], tex2[n][3]"""
        self._lib("tex_numpy")
        self._channels("tex_numpy")
        self.parent.sync()
        return self._get("tex1", 3, self.ncap, self.nn), self._get("tex2", 3, self.ncap, self.nn)

    def set_tex_numpy(self, tex1=None, tex2=None):
        self._lib("set_tex_numpy")
        self._channels("set_tex_numpy")
        arrays = {}
        for key, a in (("tex1", tex1), ("tex2", tex2)):
            if a is not None:
                a = np.asarray(a, f32).reshape(-1, 3)
                if a.shape[0] != self.nn:
                    raise RuntimeError("VortexSheetMesh::set_tex_numpy: %s has %d entries, the mesh %d nodes" % (key, a.shape[0], self.nn))
                arrays[key] = a
        for key, a in arrays.items():
            if self.nn:
                self._ch[key].view(3, self.ncap)[:, :self.nn] = torch.from_numpy(np.ascontiguousarray(a.T)).to(self.parent.device)

    def turb_numpy(self):
        """-> k[n], epsilon[n]: the TurbulenceChannel, which nothing in the reference writes"""
        self._lib("turb_numpy")
        self._channels("turb_numpy")
        self.parent.sync()
        t = self._get("turb", 2, self.ncap, self.nn)
        return t[:, 0].copy(), t[:, 1].copy()

    def getTexOffset(self):
        return self.mTexOffset

    # --- the reference's methods ---
    def calcVorticity(self):
        """vortexsheet.cpp:45-59: vorticity from circulation and the edges, per triangle; smokeAmount = 0"""
        lib = self._lib("calcVorticity")
        ch = self._channels("calcVorticity")
        lib.call("mf_vsheet_calc_vorticity", *(self._mesh_args() + (_ptr(ch["circulation"]), _ptr(ch["vorticity"]), _ptr(ch["smokeAmount"]),
                                                                 self.parent.stream)))

    def calcCirculation(self):
        raise RuntimeError("VortexSheetMesh::calcCirculation: not implemented in mantaflow_amd (its body is the reference's generated closed "
                           "form SolveOverconstraint34, which has no statement of its own here; circulation is a settable channel)")

    def reinitTexCoords(self):
        """vortexsheet.cpp:78-91: tex1 = tex2 = pos + mTexOffset"""
        lib = self._lib("reinitTexCoords")
        ch = self._channels("reinitTexCoords")
        o = self.mTexOffset
        lib.call("mf_vsheet_reinit_tex", self.nn, self.ncap, _ptr(self.pos), o[0], o[1], o[2], _ptr(ch["tex1"]), _ptr(ch["tex2"]), self.parent.stream)


def _sheet(mesh):
    if not isinstance(mesh, VortexSheetMesh):
        raise RuntimeError("can't convert argument to VortexSheetMesh*")
    return mesh


def _first_solver(mesh, name):
    """the refusals by name come before the argument checks; they need a solver, which any solver-owned first argument has"""
    s = getattr(mesh, "parent", None)
    if s is None or not hasattr(s, "_slab_window"):
        raise RuntimeError("can't convert argument to VortexSheetMesh*")
    return _sheet_lib(s, name)


@plugin
def meshSmokeInflow(mesh, shape, amount):
    """vortexplugins.cpp:69-75: smokeAmount = amount on the triangles whose face centre is inside the shape"""
    lib = _first_solver(mesh, "meshSmokeInflow")
    _sheet(mesh)
    kind, q = _shape_record("meshSmokeInflow", shape)
    amount = _real(amount)
    ch = mesh._channels("meshSmokeInflow")
    lib.call("mf_vsheet_smoke_inflow", *(mesh._mesh_args() + (kind, q, amount, _ptr(ch["smokeAmount"]), mesh.parent.stream)))


@plugin
@real_parameters("maxAmount")
def vorticitySource(mesh, gravity, vel=None, velOld=None, scale=0.1, maxAmount=0, mult=1.0):
    """vortexplugins.cpp:83-120: buoyancy adds vorticity, -cross(faceNormal, a - gravity) * scale * dt / dx per triangle with a the
    acceleration (vel - velOld) / dt sampled at the face centre (absent without vel); triangles with a fixed node get none; |vorticity|
    is clamped to maxAmount where that is positive.  The acceleration grid comes from the solver's pool and returns to it."""
    lib = _first_solver(mesh, "vorticitySource")
    _sheet(mesh)
    g = _to_vec3(gravity)
    s = mesh.parent
    for v in (vel, velOld):
        if v is not None and not isinstance(v, MACGrid):
            raise RuntimeError("can't convert argument to MACGrid*")
    if vel is not None and velOld is None:
        raise RuntimeError("vorticitySource: vel needs velOld")       # the reference dereferences the null pointer
    for v in (vel, velOld):
        if v is not None and (v.parent.device != s.device or tuple(v.dims) != tuple(s.mGridSize)):
            raise RuntimeError("vorticitySource: the velocity grids must be of the mesh's solver's size and device")
    scale, maxAmount, mult = _real(scale), _real(maxAmount), _real(mult)
    ch = mesh._channels("vorticitySource")
    dt = f32(s.getDt())
    dx = f32(s.getDx())
    sx, sy, sz = s.mGridSize
    accel = s._alloc("vec", zero=False) if vel is not None else None
    norms, release = mesh._meshops_scratch(4 * max(mesh.nt, 1))
    try:
        if vel is not None:
            lib.call("mf_vsheet_acceleration", sx, sy, sz, vel.ptr, velOld.ptr, float(f32(1.0 / float(dt))), _ptr(accel), s.stream)
        out = (ctypes.c_double * 2)()
        lib.call("mf_vsheet_source", sx, sy, sz, _ptr(accel), *(mesh._mesh_args() + (_ptr(mesh.nflag), float(f32(g.x)), float(f32(g.y)), float(f32(g.z)),
                 scale, maxAmount, mult, float(dt), float(dx), _ptr(ch["vorticity"]), _ptr(norms), out, s.stream)))
    finally:
        release()
        if accel is not None:
            s._release("vec", accel)
    # 0 / 0 triangles prints nan in the reference
    _stats["source"] = dict(max=float(out[0]), mean=(float(out[1]) / mesh.nt) if mesh.nt else float("nan"))


def _smooth_mult(sigma):
    """const Real mult = -0.5 / sigma / sigma: double divisions of the float sigma, rounded once"""
    return float(f32((-0.5 / float(f32(sigma))) / float(f32(sigma))))


@plugin
def smoothVorticity(mesh, iter=1, sigma=0.2, alpha=0.8):
    """vortexplugins.cpp:122-166: vorticitySmoothed = alpha * (`iter` Jacobi passes of a Gaussian-weighted average over the three edge
    neighbours) of vorticity.  The corner table is the mesh's cached one; the weight table and the two pass buffers come from the solver's
    pool where they fit."""
    lib = _first_solver(mesh, "smoothVorticity")
    _sheet(mesh)
    sigma, alpha = _real(sigma), _real(alpha)
    ch = mesh._channels("smoothVorticity")
    s = mesh.parent
    if mesh.nt == 0:
        return
    _extension_lib(s, "smoothVorticity", "meshops")
    conn = mesh._connectivity(lib, "smoothVorticity")
    nt = max(mesh.nt, 1)
    taken = [mesh._meshops_scratch(b) for b in (12 * nt, 12 * nt, 12 * nt, 12 * nt)]
    (w, _), (idx, _), (t0, _), (t1, _) = taken
    try:
        lib.call("mf_vsheet_smooth_weights", *(mesh._mesh_args() + (_ptr(conn["opposite"]), _smooth_mult(sigma), _ptr(w), _ptr(idx), s.stream)))
        lib.call("mf_vsheet_smooth_iterate", mesh.nt, mesh.tcap, _ptr(w), _ptr(idx), iter, alpha, _ptr(ch["vorticity"]), _ptr(ch["vorticitySmoothed"]),
                 _ptr(t0), _ptr(t1), s.stream)
    finally:
        for _, release in taken:
            release()


@plugin
def texcoordInflow(mesh, shape, vel):
    """vortexplugins.cpp:41-66: the process-wide offset t0 moves against the mean velocity of the cells inside the shape, becomes the
    mesh's reference offset, and the nodes inside the shape get tex1 = tex2 = pos + t0.  Precondition (the reference reads outside the
    velocity grid there): no cell of the last z plane is inside the shape; refused with everything unchanged.  The marks, the list of
    samples and the scan's workspace come from the solver's pool and return to it; 16 bytes cross to the host."""
    lib = _first_solver(mesh, "texcoordInflow")
    _sheet(mesh)
    kind, q = _shape_record("texcoordInflow", shape)
    if not isinstance(vel, MACGrid):
        raise RuntimeError("can't convert argument to MACGrid*")
    s = mesh.parent
    if vel.parent.device != s.device or tuple(vel.dims) != tuple(s.mGridSize):
        raise RuntimeError("texcoordInflow: the velocity grid must be of the mesh's solver's size and device")
    ch = mesh._channels("texcoordInflow")
    need = ctypes.c_int64(0)
    lib.call("mf_vsheet_inflow_tmp_bytes", vel.sx, vel.sy, vel.sz, ctypes.byref(need))
    mark, values = s._alloc("int", zero=False), s._alloc("vec", zero=False)       # the marks and the list of samples: pool grids
    tmp, release = mesh._meshops_scratch(need.value)
    out = (ctypes.c_float * 4)()
    t0 = _state.t0
    try:
        lib.call("mf_vsheet_inflow_mean", vel.sx, vel.sy, vel.sz, vel.ptr, kind, q, t0[0], t0[1], t0[2], float(f32(s.getDt())), _ptr(mark), _ptr(values),
                 _ptr(tmp), tmp.numel() * tmp.element_size(), out, s.stream)
    finally:
        release()
        s._release("vec", values)
        s._release("int", mark)
    if out[3] != 0.0:
        raise RuntimeError("texcoordInflow: the shape contains cells of the last z plane, where getCentered reads outside the velocity grid")
    _state.t0 = t0 = (float(out[0]), float(out[1]), float(out[2]))
    mesh.mTexOffset = t0                      # setReferenceTexOffset
    lib.call("mf_vsheet_inflow_apply", mesh.nn, mesh.ncap, _ptr(mesh.pos), kind, q, t0[0], t0[1], t0[2], _ptr(ch["tex1"]), _ptr(ch["tex2"]), s.stream)


@plugin
def VICintegration(mesh, sigma, vel, flags, vorticity=None, cgMaxIterFac=1.5, cgAccuracy=1e-3, scale=0.01, precondition=0):
    """vortexplugins.cpp:192-295, vortex-in-cell integration: the sheet's vorticity is spread onto the grid with a normalised Peskin
    kernel of radius sigma (order-exact: a cell adds its triangles in ascending triangle number), then the vector Poisson equation
    laplace(psi) = curl(vort) is solved per component with the library's PCG (L2 norm, MIC(0)), and vel = scale * psi.  precondition
    follows the reference: 2 (PC_mICP) runs; 0 and 3 raise its assertion -- so its own default fails; 1 (PC_ICP) is not implemented.
    Precondition: no face centre whose float sum `pos + i` rounds onto the grid size (the reference addresses a cell outside the grid
    there; the device leaves that cell out).  Grids come from the solver's pool and return to it."""
    lib = _first_solver(mesh, "VICintegration")
    _sheet(mesh)
    sigma = _real(sigma)
    if not isinstance(vel, VecGrid):
        raise RuntimeError("can't convert argument to Grid<Vec3>")
    if not isinstance(flags, FlagGrid):
        raise RuntimeError("can't convert argument to FlagGrid")
    if vorticity is not None and (not isinstance(vorticity, VecGrid) or isinstance(vorticity, MACGrid)):
        raise RuntimeError("can't convert argument to Grid<Vec3>*")
    cgMaxIterFac, cgAccuracy, scale = _real(cgMaxIterFac), _real(cgAccuracy), _real(scale)
    s = mesh.parent
    for g in (vel, flags, vorticity):
        if g is not None and (g.parent.device != s.device or tuple(g.dims) != tuple(s.mGridSize)):
            raise RuntimeError("VICintegration: the grids must be of the mesh's solver's size and device")
    if precondition == 1:
        raise RuntimeError("VICintegration: the plain incomplete-Cholesky preconditioner (precondition=1) is not implemented")
    if precondition != 2:
        raise RuntimeError("GridCg<APPLYMAT>::setICPreconditioner: Invalid method specified.")      # conjugategrad.cpp:312
    if not sigma > 0:
        raise RuntimeError("VICintegration: sigma must be positive")
    ch = mesh._channels("VICintegration")
    sx, sy, sz = s.mGridSize
    st = s.stream
    need = ctypes.c_int64(0)
    lib.call("mf_vsheet_spread_tmp_bytes", sx, sy, sz, sigma, mesh.nt, ctypes.byref(need))
    vort = vorticity if vorticity is not None else VecGrid(s)
    tmp, release = mesh._meshops_scratch(need.value)
    wnorm, release_w = mesh._meshops_scratch(4 * max(mesh.nt, 1))
    try:
        lib.call("mf_vsheet_spread", sx, sy, sz, flags.ptr, *(mesh._mesh_args() + (_ptr(ch["vorticity"]), sigma, _ptr(wnorm), vort.ptr, _ptr(tmp),
                 tmp.numel() * tmp.element_size(), st)))
    finally:
        release_w()
        release()
    _stats["vic"] = _vic_solve(lib, s, vort, vel, flags, cgMaxIterFac, cgAccuracy, scale)


_vic_keep = None      # tests set a list: each component appends its right-hand side as a numpy copy


def _vic_solve(lib, s, vort, vel, flags, cgMaxIterFac, cgAccuracy, scale):
    """vortexplugins.cpp:250-294: MakeLaplaceMatrix, CurlOp, and per component the rhs (one grid reused: the shifted form leaves its
    border as the previous component left it), a CG solve from a cleared solution (L2 norm, PC_mICP) and vel[c] = solution * scale.
    solvePressureSystem's pressure fixing is not part of this.  -> per component the iterations and the final residual"""
    sx, sy, sz = s.mGridSize
    st = s.stream
    curl = VecGrid(s)
    rhs, solution, residual, search, temp1, A0, Ai, Aj, Ak, pca0 = (Grid(s) for _ in range(10))
    lib.call("mf_make_laplace_matrix", sx, sy, sz, flags.ptr, A0.ptr, Ai.ptr, Aj.ptr, Ak.ptr, None, st)
    lib.call("mf_vsheet_curl", sx, sy, sz, vort.ptr, curl.ptr, st)
    maxIter = int(f32(cgMaxIterFac) * f32(max(sx, sy, sz)))
    shifted = int(isinstance(vel, MACGrid))
    stats = []
    for c in range(3):
        lib.call("mf_vsheet_rhs", sx, sy, sz, curl.ptr, rhs.ptr, c, shifted, st)
        if _vic_keep is not None:
            s.sync()
            _vic_keep.append(rhs.data.cpu().numpy().copy())
        out = (ctypes.c_float * 3)()
        lib.call("mf_cg_solve", sx, sy, sz, flags.ptr, solution.ptr, rhs.ptr, residual.ptr, search.ptr, temp1.ptr, A0.ptr, Ai.ptr, Aj.ptr, Ak.ptr,
                 pca0.ptr, 2, cgAccuracy, maxIter, 1, out, st)
        lib.call("mf_vsheet_set_component", sx, sy, sz, vel.ptr, solution.ptr, scale, c, st)
        stats.append(dict(iterations=int(out[0]), residual=float(out[2])))
    return stats
