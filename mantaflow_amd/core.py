"""Host-side mirror of the reference's object model for the hot path.

Mirrors (names, argument meaning, defaults, error behaviour) of:
  FluidSolver / Solver           source/fluidsolver.{h,cpp}
  Grid<T>, MACGrid, FlagGrid     source/grid.{h,cpp}
  LevelsetGrid                   source/levelset.h (container + join/subtract only)
  BasicParticleSystem, Pdata*    source/particle.{h,cpp}
  vec3                           source/pwrapper/pvec3.cpp
Storage is a torch tensor on the active library's device (``cuda`` for the HIP product library); all arithmetic on
the hot path goes through the C ABI (mantaflow_amd._lib).  Grids are dense, x fastest; Vec3/MAC grids and particle
vectors are structure-of-arrays ([3][N]); the reference's AoS [z][y][x][3] view exists only at the numpy bridge.
"""
import ctypes
import os
import ctypes.util
import gzip
import math
import re
import struct

import functools
import types

import numpy as np
import torch

from . import _lib, fileio

# ---------------------------------------------------------------------------------------------------------
# constants: FlagGrid::CellType (grid.h:306-320), particle status (particle.h:34-43), python/defines.py:25-60
# ---------------------------------------------------------------------------------------------------------
TypeNone, TypeFluid, TypeObstacle, TypeEmpty, TypeInflow, TypeOutflow, TypeOpen, TypeStick = 0, 1, 2, 4, 8, 16, 32, 64
TypeSurface, TypeReserved, TypeBandInterface, TypeTemp = 128, 256, 512, 32768
PNONE, PNEW, PSPRAY, PBUBBLE, PFOAM, PTRACER, PDELETE, PINVALID = 0, 1, 2, 4, 8, 16, 1 << 10, 1 << 30
VECTOR_EPSILON = 1e-6


class vec3(object):
    """manta.vec3 -- float[3] with component-wise + - * / against vec3 or scalar (pvec3.cpp:40-145)."""
    __slots__ = ("x", "y", "z")

    def __init__(self, x=None, y=None, z=None):
        if x is None:
            x = y = z = 0.0
        elif isinstance(x, (vec3, tuple, list)) and y is None:
            x, y, z = (x.x, x.y, x.z) if isinstance(x, vec3) else x
        elif y is None:
            y = z = x
        elif z is None:
            raise TypeError("vec3 takes 0, 1 or 3 numbers")
        self.x, self.y, self.z = float(np.float32(x)), float(np.float32(y)), float(np.float32(z))

    @staticmethod
    def _c(o):
        return o if isinstance(o, vec3) else vec3(o) if isinstance(o, (int, float, tuple, list, np.number)) else None

    def _bin(self, o, f):
        o = vec3._c(o)
        if o is None:
            return NotImplemented
        return vec3(f(self.x, o.x), f(self.y, o.y), f(self.z, o.z))

    def __add__(self, o): return self._bin(o, lambda a, b: a + b)
    def __sub__(self, o): return self._bin(o, lambda a, b: a - b)
    def __mul__(self, o): return self._bin(o, lambda a, b: a * b)
    def __truediv__(self, o): return self._bin(o, lambda a, b: a / b)
    def __radd__(self, o): return vec3._c(o)._bin(self, lambda a, b: a + b)
    def __rsub__(self, o): return vec3._c(o)._bin(self, lambda a, b: a - b)
    def __rmul__(self, o): return vec3._c(o)._bin(self, lambda a, b: a * b)
    def __rtruediv__(self, o): return vec3._c(o)._bin(self, lambda a, b: a / b)
    def __neg__(self): return vec3(-self.x, -self.y, -self.z)
    def __iter__(self): return iter((self.x, self.y, self.z))
    def __getitem__(self, i): return (self.x, self.y, self.z)[i]
    def __eq__(self, o):
        o = vec3._c(o)
        return o is not None and (self.x, self.y, self.z) == (o.x, o.y, o.z)
    def __repr__(self): return "[%+4.6f,%+4.6f,%+4.6f]" % (self.x, self.y, self.z)
    def max(self): return max(self.x, self.y, self.z)


class vec4(object):
    """manta.vec4 (pvec3.cpp:280-389): float[4] with members x, y, z, t; built from nothing (zeros), one number (broadcast) or four;
    unlike vec3 it has no arithmetic (tp_as_number is NULL in the reference)"""
    __slots__ = ("x", "y", "z", "t")

    def __init__(self, x=None, y=None, z=None, t=None):
        if x is None:
            if not (y is None and z is None and t is None):
                raise RuntimeError("Invalid partial init of vec4")
            x = y = z = t = 0.0
        elif y is None and z is None and t is None:
            y = z = t = x
        elif y is None or z is None or t is None:
            raise RuntimeError("Invalid partial init of vec4")
        self.x, self.y, self.z, self.t = (float(np.float32(v)) for v in (x, y, z, t))

    def __iter__(self): return iter((self.x, self.y, self.z, self.t))
    def __getitem__(self, i): return (self.x, self.y, self.z, self.t)[i]
    def __repr__(self): return "[%+4.6f,%+4.6f,%+4.6f,%+4.6f]" % (self.x, self.y, self.z, self.t)


def _to_vec3(v, what="Vec3"):
    if isinstance(v, vec3):
        return v
    if isinstance(v, (tuple, list)) and len(v) == 3:
        return vec3(*v)
    raise RuntimeError("can't convert argument to %s" % what)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    if dev == "cuda" or (isinstance(dev, str) and dev.startswith("cuda")):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return None


def _method_kwargs(fn):
    """every PYTHON() member accepts the universal `notiming` / `nocheck` keywords (codegen_python.cpp:37, pconvert.cpp:461)"""
    @functools.wraps(fn)
    def w(self, *a, **kw):
        kw.pop("notiming", None)
        kw.pop("nocheck", None)
        return fn(self, *a, **kw)
    return w


def _extension_lib(s, name, ext):
    """the solver's library, if plugin or method `name` of extension `ext` (a row of _lib.EXTENSIONS, by name) can run on it; refused
    before any grid is touched: a z-slab solver first, then a backend without the extension (the CPU test backend has none)"""
    ext = _lib.extension(ext)
    if tuple(s._slab_window) != (0, 0):
        raise RuntimeError("%s: %s %s not run on a z-slab solver" % (name, ext.what, ext.verb))
    if not getattr(s.lib, ext.name):
        raise RuntimeError(ext.not_implemented(name, s.lib.backend))
    return s.lib


# the numpy bridge of every container: storage is component planes ([ncomp][elements], x fastest), the arrays carry an element's
# components together ([shape] for one component, [shape][ncomp] for more)
def _planes_to_elements(planes, shape):
    """a copy of `planes` ([ncomp][elements], any strides) as the bridge's array"""
    if len(planes) == 1:
        return planes[0].reshape(shape).copy()
    return np.ascontiguousarray(planes.T).reshape(shape + (len(planes),))


def _elements_to_planes(arr, shape, ncomp):
    """the bridge's array as contiguous planes [ncomp][elements]"""
    arr = np.asarray(arr)
    if ncomp == 1:
        return np.ascontiguousarray(arr.reshape(math.prod(shape)))[None]
    return np.ascontiguousarray(arr.reshape(shape + (ncomp,)).reshape(math.prod(shape), ncomp).T)


def _format_element(is_int, ncomp, component="%+4.2f"):
    """how the reference's streams print one element: %d, %g, or a vector's components in brackets"""
    if is_int:
        return lambda v: "%d" % v
    if ncomp == 1:
        return lambda v: "%g" % v
    return lambda v: "[" + ",".join(component % x for x in v) + "]"


class PbClass(object):
    """Base of every solver-owned object (pwrapper/pclass.h): parent solver + name."""
    _T = ""

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        for name, attr in list(cls.__dict__.items()):
            if isinstance(attr, types.FunctionType) and not name.startswith("_"):
                setattr(cls, name, _method_kwargs(attr))

    def __init__(self, parent, name=""):
        if parent is None:
            raise RuntimeError("New class %s: no parent given -- specify using parent=xxx !" % type(self).__name__)
        self.parent = parent
        self.name = name or ""

    def getParent(self): return self.parent
    def setName(self, n): self.name = n
    def getName(self): return self.name
    # introspection attributes of every wrapped object (registry.cpp:123-133, 320-326): C class name without / with template
    @property
    def _class(self): return type(self)._cname_cpp
    @property
    def _cname(self):
        t = getattr(type(self), "_T", "")
        return type(self)._cname_cpp + ("<%s>" % t if t else "")


class SolverLib(object):
    """The C ABI as seen by ONE solver: every call is made under that solver's z-slab window (zoff, gsz) -- (0, 0) for an
    ordinary solver whose grids are the whole domain.  The window is thread-local state of the library; binding it to the
    solver means a slab solver and a plain solver (or two slab solvers of different resolution, as in waveletTurbulence.py) can
    live in one process without inheriting each other's coordinates."""

    def __init__(self, lib, solver):
        self._lib, self._solver = lib, solver
        self.backend, self.device, self.cdll, self.path = lib.backend, lib.device, lib.cdll, lib.path
        for ext in _lib.all_extensions():
            setattr(self, ext.name, getattr(lib, ext.name))

    def call(self, name, *args):
        # set on every call: the window is thread-local state of the shared object, so a cache per Library object would go
        # stale under a second host thread or a second Library on the same .so (two thread-local stores per call)
        lib, w = self._lib, self._solver._slab_window
        lib.cdll.mf_set_slab_window(w[0], w[1])
        return lib.call(name, *args)

    def call2(self, src_solver, name, *args):
        """a call that reads a grid of another solver (interpolateGrid & co.): that grid's window goes in as the source window"""
        lib, w = self._lib, src_solver._slab_window
        lib.cdll.mf_set_slab_window_source(w[0], w[1])
        return self.call(name, *args)


# ---------------------------------------------------------------------------------------------------------
# FluidSolver (python name Solver), fluidsolver.{h,cpp}
# ---------------------------------------------------------------------------------------------------------
class FluidSolver(PbClass):
    _cname_py, _cname_cpp = "Solver", "FluidSolver"

    def __init__(self, gridSize, dim=3, fourthDim=-1, name="", **kw):
        gs = _to_vec3(gridSize, "Vec3i")
        self.mGridSize = (int(gs.x), int(gs.y), int(gs.z))
        if dim not in (2, 3):
            raise RuntimeError("Only 2D and 3D solvers allowed.")
        if dim == 2 and self.mGridSize[2] != 1:
            raise RuntimeError("Trying to create 2D solver with size.z != 1")
        self.mDim = dim
        self.mFourthDim = int(fourthDim)
        PbClass.__init__(self, self, name)
        # fluidsolver.cpp:106-109
        self.timestep = 1.0
        self.timeTotal = 0.0
        self.frame = 0
        self.mCount = 0
        self.cfl = 1000.0
        self.timestepMin = 1.0
        self.timestepMax = 1.0
        self.frameLength = 1.0
        self.timePerFrame = 0.0
        self.mLockDt = False
        self._slab_window = (0, 0)
        self._mg = None    # the GridMg of solvePressure(preconditioner=PcMGStatic | PcMGDynamic): one per solver (pressure.cpp:245-248)
        self.lib = SolverLib(_lib.get(), self)
        self.device = self.lib.device
        self._pool = {}    # dtype/ncomp -> list of free tensors  (GridStorage, fluidsolver.cpp:34-50)
        self._pool4 = {}   # the same for the 4-D grids (mGrids4d*, fluidsolver.h): kind -> list of free tensors
        self._reinit_ctr = None    # the eight device counters of LevelsetGrid.reinitMarching
        self._live = 0
        self.timings = {}

    # --- accessors ---
    def getGridSize(self): return vec3(*self.mGridSize)
    def is2D(self): return self.mDim == 2
    def is3D(self): return self.mDim == 3
    def supports4D(self): return self.mFourthDim > 0
    def getFourthDim(self): return self.mFourthDim
    def getDt(self): return float(np.float32(self.timestep))
    def globalGridSize(self):
        """size of the whole domain: mGridSize, or -- for the solver of a z-slab (slab.SlabDomain) -- the undivided grid's"""
        return getattr(self, "_global_size", None) or self.mGridSize
    def getDx(self): return 1.0 / max(self.globalGridSize())   # a z-slab reports the whole domain's dx
    @property
    def ncells(self): return self.mGridSize[0] * self.mGridSize[1] * self.mGridSize[2]
    @property
    def stream(self): return _stream(self.device)

    # --- temp-grid pool: LIFO stack per element type; freshly handed grids are zeroed (grid.cpp:49-60) ---
    def _alloc(self, kind, zero=True):
        ncomp, dtype = (3, torch.float32) if kind == "vec" else ((1, torch.int32) if kind == "int" else (1, torch.float32))
        free = self._pool.setdefault(kind, [])
        if free:
            t = free.pop()
            if zero:
                t.zero_()
        else:
            if self._live > 200:
                raise RuntimeError("too many temp grids used -- are they released properly ?")
            t = torch.zeros(ncomp * self.ncells, dtype=dtype, device=self.device)
        self._live += 1
        return t

    def _release(self, kind, t):
        self._live -= 1
        self._pool.setdefault(kind, []).append(t)

    # --- the 4-D pool (getGrid4dPointer / freeGrid4dPointer): the same stack per element type, beside the 3-D one ---
    def _alloc4(self, kind):
        ncomp = {"real": 1, "int": 1, "vec3": 3, "vec4": 4}[kind]
        free = self._pool4.setdefault(kind, [])
        if free:
            t = free.pop()
            t.zero_()
        else:
            if self._live > 200:
                raise RuntimeError("too many temp grids used -- are they released properly ?")
            t = torch.zeros(ncomp * self.ncells * self.mFourthDim, dtype=torch.int32 if kind == "int" else torch.float32, device=self.device)
        self._live += 1
        return t

    def _release4(self, kind, t):
        self._live -= 1
        self._pool4.setdefault(kind, []).append(t)

    # --- time stepping, fluidsolver.cpp:143-204 ---
    def step(self, frame=-1):
        self.timePerFrame = float(np.float32(self.timePerFrame + self.timestep))
        self.timeTotal = float(np.float32(self.timeTotal + self.timestep))
        self.mCount += 1
        if (self.timePerFrame + VECTOR_EPSILON) > self.frameLength:
            self.frame += 1
            self.timeTotal = float(self.frame) * self.frameLength
            self.timePerFrame = 0.0
            self.mLockDt = False
        if frame >= 0:
            self.frame = frame

    def adaptTimestep(self, maxVel):
        f32 = np.float32
        mvt = f32(maxVel) * f32(self.timestep)
        if not self.mLockDt:
            dt = f32(f32(self.timestep) * f32(float(f32(self.cfl)) / (float(mvt) + 1e-05)))      # mCflCond is a Real: Real / double
            dt = max(min(dt, f32(self.timestepMax)), f32(self.timestepMin))
            if (self.timePerFrame + float(dt) * 1.05) > self.frameLength:
                dt = f32((self.frameLength - self.timePerFrame) + 1e-04)
            elif (self.timePerFrame + float(dt) + self.timestepMin) > self.frameLength or \
                    (self.timePerFrame + (float(dt) * 1.25)) > self.frameLength:
                dt = f32((self.frameLength - self.timePerFrame + 1e-04) * 0.5)
                self.mLockDt = True
            self.timestep = float(dt)
        if not (self.timestep > (self.timestepMin / 2.)):
            raise RuntimeError("Invalid dt encountered! Shouldnt happen...")

    def printMemInfo(self):
        print("Allocated grids: %s live, pooled %s" % (self._live, {k: len(v) for k, v in self._pool.items()}))

    def create(self, type, name="", **kw):
        """Solver.create(Type, ...) -> object with this solver as parent (fluidsolver.cpp:129-140)."""
        if not callable(type):
            raise RuntimeError("can't convert argument to PbType")
        return type(parent=self, name=name, **kw)

    def sync(self):
        if self.device != "cpu":
            torch.cuda.current_stream().synchronize()


Solver = FluidSolver


# ---------------------------------------------------------------------------------------------------------
# grids, grid.{h,cpp}
# ---------------------------------------------------------------------------------------------------------
class GridBase(PbClass):
    TypeNone, TypeReal, TypeInt, TypeVec3, TypeMAC, TypeLevelset, TypeFlags = 0, 1, 2, 4, 8, 16, 32
    _kind, _ncomp = "real", 1

    def __init__(self, parent, show=True, name="", **kw):
        PbClass.__init__(self, parent, name)
        s = parent
        self.sx, self.sy, self.sz = s.mGridSize
        self.n = self.sx * self.sy * self.sz
        self.data = s._alloc(self._kind)       # zeroed (Grid ctor calls clear(), grid.cpp:58)
        self._external = False

    def __del__(self):
        try:
            if not self._external and self.data is not None:
                self.parent._release(self._kind, self.data)   # release stores the *current* pointer (post-swap)
        except Exception:
            pass

    # geometry
    def getSizeX(self): return self.sx
    def getSizeY(self): return self.sy
    def getSizeZ(self): return self.sz
    def getSize(self): return vec3(self.sx, self.sy, self.sz)
    def is3D(self): return self.parent.is3D()
    def is4D(self): return False
    def getDx(self): return 1.0 / max(self.parent.globalGridSize())
    def getType(self): return self._gtype
    def getGridType(self): return self._gtype
    @property
    def dims(self): return (self.sx, self.sy, self.sz)
    @property
    def ptr(self): return _ptr(self.data)
    def _call(self, fn, *args): return self.parent.lib.call(fn, *args)

    def _check_same(self, o):
        if (o.sx, o.sy, o.sz) != (self.sx, self.sy, self.sz):
            raise RuntimeError("different grid resolutions [%d,%d,%d] vs [%d,%d,%d]" % (o.sx, o.sy, o.sz, self.sx, self.sy, self.sz))

    # element-wise API of Grid<T> (grid.h:113-180, grid.cpp:228-330)
    def clear(self):
        self._call("mf_fill_f32", self.data.numel(), self.ptr, 0.0, self.parent.stream)

    def copyFrom(self, a, copyType=True):
        self._check_same(a)
        self._call("mf_copy_f32", self.data.numel(), self.ptr, a.ptr, self.parent.stream)
        return self

    def swap(self, other):
        """pointer swap, grid.cpp:100-111"""
        self._check_same(other)
        self.data, other.data = other.data, self.data

    def getDataPointer(self): return "%x" % self.data.data_ptr()

    def setBoundNeumann(self, boundaryWidth):
        """Grid<T>::setBoundNeumann -> knSetBoundaryNeumann, grid.cpp:640-669: every cell within boundaryWidth + 1 of a side takes
        the value of the nearest cell inside (per component: the words are copied)"""
        w = int(boundaryWidth)
        lo = 2 * w + 3
        if w < 0 or self.sx < lo or self.sy < lo or (self.is3D() and self.sz < lo):
            raise RuntimeError("setBoundNeumann: grid [%d,%d,%d] too small for boundaryWidth %d" % (self.sx, self.sy, self.sz, w))
        lib = self.parent.lib
        if lib.resample:
            for c in range(self._ncomp):
                self._call("mf_grid_set_bound_neumann", self.sx, self.sy, self.sz, _ptr(self.data[c * self.n:]), w, self.parent.stream)
            return
        if lib.backend == "hip":
            raise RuntimeError("setBoundNeumann: %s lacks the resampling extension (manta_hip_resample.h) -- rebuild the library" % lib.path)
        # the CPU checker backend: the same separable index map as a torch expression
        dev = self.data.device
        def src(size):
            i = torch.arange(size, device=dev)
            i = torch.where(i <= w, torch.full_like(i, w + 1), i)
            return torch.where(torch.arange(size, device=dev) >= size - 1 - w, torch.full_like(i, size - w - 2), i)
        v = self.data.view(self._ncomp, self.sz, self.sy, self.sx)
        if self.is3D():
            v = v.index_select(1, src(self.sz))
        self.data.copy_(v.index_select(2, src(self.sy)).index_select(3, src(self.sx)).reshape(-1))

    # host-only accessors (grid.h:34-35, 83-84; Grid<T>::get / set): no kernel, every backend
    def get_name(self): return self.getName()
    def set_name(self, s): self.setName(s)
    def getSizeT(self): return 1
    def getStrideT(self): return 0

    def _checked_index(self, what, i, j, k):
        """the linear index of cell (i, j, k), refused outside the grid (GridBase::checkIndex, grid.h:56)"""
        i, j, k = int(i), int(j), int(k)
        if not (0 <= i < self.sx and 0 <= j < self.sy and 0 <= k < self.sz):
            raise RuntimeError("Grid::%s: index %d,%d,%d out of bound [%d,%d,%d]" % (what, i, j, k, self.sx, self.sy, self.sz))
        return i + self.sx * (j + self.sy * k)

    def _words(self, idx):
        """the element at a linear index, read back: one value per component plane"""
        self.parent.sync()
        return [self.data[c * self.n + idx].item() for c in range(self._ncomp)]

    def get(self, i, j, k):
        """Grid<T>::get(i, j, k): one element read back to the host (an int, a float or a vec3)"""
        w = self._words(self._checked_index("get", i, j, k))
        return vec3(*w) if self._ncomp == 3 else w[0]

    def set(self, i, j, k, val):
        """Grid<T>::set(i, j, k, val): one element written from the host"""
        idx = self._checked_index("set", i, j, k)
        if self._ncomp == 3:
            v = _to_vec3(val)
            for c, x in enumerate((v.x, v.y, v.z)):
                self.data[c * self.n + idx] = float(np.float32(x))
        else:
            self.data[idx] = int(val) if self._kind == "int" else float(np.float32(val))

    @staticmethod
    def _interpol_axis(p, size, clamp_on_index, cut_upper=True):
        """one axis of BUILD_INDEX (p = pos - 0.5, util/interpol.h:52-67) or of its shifted half (p = pos, :116-129): the base index
        and the fp32 weights (w0, w1); `1. - w1` is a double difference rounded once.  The upper clamp tests p itself in BUILD_INDEX
        and the truncated index in the shifted half; a 2-D grid's z axis has no upper clamp."""
        f32 = np.float32
        p = f32(p)
        if not np.isfinite(p) or abs(float(p)) >= 2.0 ** 31:
            raise RuntimeError("Grid::getInterpolated: position %r cannot be truncated to a cell" % float(p))
        i = int(p)                                          # (int): toward zero
        w1 = f32(p - f32(i))
        w0 = f32(1. - float(w1))
        if p < 0:
            i, w0, w1 = 0, f32(1), f32(0)
        if cut_upper and ((i >= size - 1) if clamp_on_index else (p >= f32(size - 1))):
            i, w0, w1 = size - 2, f32(0), f32(1)
        return i, w0, w1

    def _interpolated(self, pos, mac):
        """interpol<T> (util/interpol.h:71-82) per component, or interpolMAC (:131-164): eight elements per component read back, the
        reference's association order in fp32.  Where the reference's base index leaves the array (interpolMAC on a 2-D grid with a
        large z: it multiplies the z index by size.y, not by the z stride) the call is refused."""
        f32 = np.float32
        p = _to_vec3(pos)
        sx, sy, sz = self.dims
        z3 = self.is3D()
        Z = sx * sy if z3 else 0                             # mStrideZ
        ax = [self._interpol_axis(f32(q) - f32(0.5), n, False, c < 2 or sz > 1) for c, (q, n) in enumerate(zip((p.x, p.y, p.z), self.dims))]
        sh = [self._interpol_axis(q, n, True, c < 2 or sz > 1) for c, (q, n) in enumerate(zip((p.x, p.y, p.z), self.dims))] if mac else ax
        self.parent.sync()
        out = []
        for c in range(self._ncomp):
            # the axis that takes the shifted index and weights: component c of a MAC grid, none otherwise
            (xi, s0, s1), (yi, t0, t1), (zi, f0, f1) = [(sh if (mac and a == c) else ax)[a] for a in range(3)]
            base = (zi * sy + yi) * sx + xi if mac else xi + sx * yi + Z * zi
            if base < 0 or base + 1 + sx + Z > self.n - 1:
                raise RuntimeError("Grid::getInterpolated: position [%g,%g,%g] out of bound [%d,%d,%d]" % (p.x, p.y, p.z, sx, sy, sz))
            d = self.data[c * self.n:(c + 1) * self.n]
            r = lambda o: f32(d[base + o].item())
            a = f32(f32(f32(r(0) * t0) + f32(r(sx) * t1)) * s0) + f32(f32(f32(r(1) * t0) + f32(r(1 + sx) * t1)) * s1)
            b = f32(f32(f32(r(Z) * t0) + f32(r(sx + Z) * t1)) * s0) + f32(f32(f32(r(1 + Z) * t0) + f32(r(1 + sx + Z) * t1)) * s1)
            out.append(float(f32(f32(f32(a) * f0) + f32(f32(b) * f1))))
        return out

    # the grid operations of include/open/manta_hip_gridops.h: Real, int and Vec3 / MAC grids alike
    _GRIDOPS_KIND = {"real": 0, "int": 1, "vec": 2}

    def _gridops_lib(self, what):
        """_extension_lib for a grid method: z-slab first, then a backend without the extension"""
        return _extension_lib(self.parent, "Grid::" + what, "gridops")

    @staticmethod
    def _permutation(axis0, axis1, axis2):
        """the three axes, or None where the reference returns without doing anything (grid.cpp:323, 332)"""
        ax = (int(axis0), int(axis1), int(axis2))
        return ax if sorted(ax) == [0, 1, 2] else None

    def permuteAxes(self, axis0, axis1, axis2):
        """Grid<T>::permuteAxes, grid.cpp:322-330: target(s[axis0], s[axis1], s[axis2]) = self(s) into a pool scratch grid that then
        swaps storage with this grid; an invalid or repeated axis returns silently.  The grid must be cubic (square in 2-D); on a 2-D
        grid axis 2 must stay, because the reference's z stride of 0 folds every other permutation onto one row."""
        lib = self._gridops_lib("permuteAxes")
        ax = self._permutation(axis0, axis1, axis2)
        if ax is None:
            return
        s = self.parent
        if not (self.sx == self.sy and (s.is2D() or self.sy == self.sz)):
            raise RuntimeError("Grid must be cubic!")
        if s.is2D() and ax[2] != 2:
            raise RuntimeError("permuteAxes: (%d, %d, %d) moves axis 2 of a 2-D grid" % ax)
        tmp = s._alloc(self._kind, zero=False)
        try:
            lib.call("mf_gridops_permute", self.sx, self.sy, self.sz, ax[0], ax[1], ax[2], self._ncomp, self.ptr, _ptr(tmp), s.stream)
            self.data, tmp = tmp, self.data
        finally:
            s._release(self._kind, tmp)

    def permuteAxesCopyToGrid(self, axis0, axis1, axis2, out):
        """Grid<T>::permuteAxesCopyToGrid, grid.cpp:331-339, with the reference's two asserts.  Its kernel writes outside `out` for the
        two 3-cycles on a non-cubic grid (the assert asks sizeTarget[axisN] == size[N], the kernel needs sizeTarget[N] == size[axisN])
        and wherever axis 2 moves on a 2-D grid: those are refused here."""
        lib = self._gridops_lib("permuteAxesCopyToGrid")
        ax = self._permutation(axis0, axis1, axis2)
        if ax is None:
            return
        if not isinstance(out, GridBase):
            raise RuntimeError("can't convert argument to Grid*")
        if self.getGridType() != out.getGridType():
            raise RuntimeError("Grids must have same data type!")
        size, target = self.dims, out.dims
        if any(target[ax[q]] != size[q] for q in range(3)):
            raise RuntimeError("Permuted grids must have the same dimensions!")
        if (self.parent.is2D() or out.parent.is2D()) and ax[2] != 2:
            raise RuntimeError("permuteAxesCopyToGrid: (%d, %d, %d) moves axis 2 of a 2-D grid: the reference writes outside the target" % ax)
        if any(target[q] != size[ax[q]] for q in range(3)):
            raise RuntimeError("permuteAxesCopyToGrid: a cyclic permutation (%d, %d, %d) of a non-cubic grid [%d,%d,%d]: the reference "
                               "writes outside the target" % (ax + size))
        _extension_lib(out.parent, "Grid::permuteAxesCopyToGrid", "gridops")     # out's solver may be another one: no z-slab either
        if out.data.data_ptr() == self.data.data_ptr():
            raise RuntimeError("permuteAxesCopyToGrid: out must not be the grid itself")
        lib.call("mf_gridops_permute", self.sx, self.sy, self.sz, ax[0], ax[1], ax[2], self._ncomp, self.ptr, out.ptr, self.parent.stream)

    def _norm(self, what, l2, bnd):
        lib = self._gridops_lib(what)
        if int(bnd) < 0:
            raise RuntimeError("%s: bnd %d is negative: the reference reads outside the grid" % (what, int(bnd)))
        r = ctypes.c_float()
        lib.call("mf_gridops_norm", self._GRIDOPS_KIND[self._kind], l2, self.sx, self.sy, self.sz, int(bnd), self.ptr, ctypes.byref(r),
                 self.parent.stream)
        return r.value

    def getL1(self, bnd=0):
        """Grid<T>::getL1, grid.cpp:390-396, 412-414: the fp64 sum of norm(x) over the cells at least bnd from every side, as fp32; the
        sum is the device's fixed-order reduction (DESIGN.md section 25 has the bound against the reference's serial loop)"""
        return self._norm("getL1", 0, bnd)

    def getL2(self, bnd=0):
        """Grid<T>::getL2, grid.cpp:401-409, 416-418: sqrt of the fp64 sum of normSquare(x), as fp32"""
        return self._norm("getL2", 1, bnd)

    def join(self, a, keepMax=True):
        """Grid<T>::join, grid.cpp:258-268, 340-348: the larger (keepMax) or smaller of the two values per cell; for Vec3 grids every
        component becomes the larger / smaller normSquare"""
        lib = self._gridops_lib("join")
        if not isinstance(a, GridBase) or a._kind != self._kind:
            raise RuntimeError("can't convert argument to Grid*")
        self._check_same(a)
        lib.call("mf_gridops_join", self._GRIDOPS_KIND[self._kind], self.n, self.ptr, a.ptr, int(bool(keepMax)), self.parent.stream)

    def save(self, name):
        """Grid<T>::save, grid.cpp:157-179 (.uni, .raw, .npz)"""
        return _grid_save(self, str(name))

    def load(self, name):
        """Grid<T>::load, grid.cpp:135-155"""
        return _grid_load(self, str(name))

    # numpy bridge (plugin/numpyconvert.cpp:145-223): [z][y][x](,[c]) arrays
    def to_numpy(self):
        return _planes_to_elements(self.data.detach().cpu().numpy().reshape(self._ncomp, self.n), (self.sz, self.sy, self.sx))

    def from_numpy(self, arr):
        flat = _elements_to_planes(arr, (self.sz, self.sy, self.sx), self._ncomp).reshape(-1)
        t = torch.from_numpy(flat.astype(np.int32 if self._kind == "int" else np.float32, copy=False))
        self.data.copy_(t.to(self.data.device))
        return self


# ---------------------------------------------------------------------------------------------------------
# .uni / .raw grid files (fileio/iogrids.cpp:255-292, 386-513): the container is fileio's; the element array is x fastest, Vec3
# grids as 3 floats per cell.  Data format either side of the hot path.
# ---------------------------------------------------------------------------------------------------------
def _unify_grid_type(t):
    """unifyGridType, iogrids.cpp:213-221"""
    if t & GridBase.TypeReal: t |= GridBase.TypeLevelset
    if t & GridBase.TypeLevelset: t |= GridBase.TypeReal
    if t & GridBase.TypeVec3: t |= GridBase.TypeMAC
    if t & GridBase.TypeMAC: t |= GridBase.TypeVec3
    return t


def _grid_header(g, dimT):
    """the UniHeader's integers of a 3-D or 4-D grid (the two classes' Type* flags agree where they are read here)"""
    et = 0 if (g._gtype & GridBase.TypeInt) else (1 if (g._gtype & GridBase.TypeReal) else 2)
    return (g.sx, g.sy, g.sz, g._gtype, et, 4 * g._ncomp, dimT)


def _grid_save(g, name):
    ext = fileio.extension(name)
    raw = g.to_numpy().astype(np.int32 if g._kind == "int" else np.float32, copy=False).tobytes()
    if ext == ".raw":
        fileio.write(name, raw)
    elif ext == ".uni":
        fileio.write(name, raw, fileio.GRID, _grid_header(g, 0))
    elif ext == ".npz":
        np.savez_compressed(name, arr_0=g.to_numpy())
    else:
        raise RuntimeError("file '%s' filetype not supported" % name)
    return 1


def _grid_load(g, name):
    ext = fileio.extension(name)
    dt = np.int32 if g._kind == "int" else np.float32
    nbytes = 4 * g._ncomp * g.n
    shape = (g.sz, g.sy, g.sx) if g._ncomp == 1 else (g.sz, g.sy, g.sx, 3)
    if ext == ".raw":
        with fileio.Reader(name) as f:
            raw = f.payload()
        if len(raw) != nbytes:
            raise RuntimeError("can't read raw file, stream length does not match, %d vs %d" % (nbytes, len(raw)))
    elif ext == ".uni":
        with fileio.Reader(name) as f:
            ident = f.magic()
            if ident != fileio.GRID:
                raise RuntimeError("readGridUni: Unknown header '%s' " % ident.decode(errors="replace"))
            dx, dy, dz, gtype, etype, bpe, dimt = f.header(ident, "can't read file, no header present")
            if (dx, dy, dz) != (g.sx, g.sy, g.sz):
                raise RuntimeError("grid dim doesn't match, [%d,%d,%d] vs [%d,%d,%d]" % (dx, dy, dz, g.sx, g.sy, g.sz))
            if _unify_grid_type(gtype) != _unify_grid_type(g._gtype):
                raise RuntimeError("grid type doesn't match %d vs %d" % (gtype, g._gtype))
            if bpe != 4 * g._ncomp:
                raise RuntimeError("grid element size doesn't match %d vs %d" % (bpe, 4 * g._ncomp))
            raw = f.payload(nbytes)         # as much as the grid holds; a shorter stream is not told apart here
    elif ext == ".npz":
        g.from_numpy(np.load(name)["arr_0"])
        return 1
    else:
        raise RuntimeError("file '%s' filetype not supported" % name)
    g.from_numpy(np.frombuffer(raw, dtype=dt).reshape(shape).copy())
    return 1


class Grid(GridBase):
    """Grid<Real> (python: RealGrid)."""
    _kind, _ncomp, _gtype = "real", 1, GridBase.TypeReal
    _cname_py, _cname_cpp, _T = "RealGrid", "Grid", "Real"

    def setConst(self, v): self._call("mf_fill_f32", self.n, self.ptr, float(v), self.parent.stream)
    def addConst(self, v): self._call("mf_grid_add_const", self.n, self.ptr, float(v), self.parent.stream)
    def multConst(self, v): self._call("mf_grid_mult_const", self.n, self.ptr, float(v), self.parent.stream)
    def clamp(self, lo, hi): self._call("mf_grid_clamp", self.n, self.ptr, float(lo), float(hi), self.parent.stream)
    def add(self, a): self._check_same(a); self._call("mf_grid_add", self.n, self.ptr, a.ptr, self.parent.stream)
    def sub(self, a): self._check_same(a); self._call("mf_grid_sub", self.n, self.ptr, a.ptr, self.parent.stream)
    def mult(self, a): self._check_same(a); self._call("mf_grid_mult", self.n, self.ptr, a.ptr, self.parent.stream)
    def addScaled(self, a, f): self._check_same(a); self._call("mf_grid_scaled_add", self.n, self.ptr, a.ptr, float(f), self.parent.stream)
    def safeDivide(self, a): self._check_same(a); self._call("mf_grid_safe_divide", self.n, self.ptr, a.ptr, self.parent.stream)
    def stomp(self, th): self._call("mf_grid_stomp", self.n, self.ptr, float(th), self.parent.stream)

    def clamp_norm(self, val):
        """Grid<Real>::clamp_norm -> knGridClampNorm, grid.cpp:306-317: where sqrt(v * v) > val, v *= val / sqrt(v * v) in fp32
        (include/open/manta_hip_movingobs.h)"""
        lib = _extension_lib(self.parent, "Grid::clamp_norm", "movingobs")
        lib.call("mf_movingobs_clamp_norm", self.n, 1, self.ptr, float(np.float32(val)), self.parent.stream)

    def setBound(self, value, boundaryWidth=1):
        """Grid::setBound -> knSetBoundary, grid.cpp:629-637"""
        self._call("mf_grid_set_bound", self.sx, self.sy, self.sz, self.ptr, float(value), int(boundaryWidth), self.parent.stream)

    def getMaxAbs(self):
        r = ctypes.c_float()
        self._call("mf_grid_max_abs", self.n, self.ptr, ctypes.byref(r), self.parent.stream)
        return r.value

    def getInterpolated(self, pos):
        """Grid<Real>::getInterpolated -> interpol<Real>, grid.h:150, util/interpol.h:71-82: trilinear (2-D: bilinear) at a position in
        grid coordinates, clamped to the border.  Host-only: eight elements are read back."""
        return self._interpolated(pos, False)[0]

    def _minmax(self):
        lo, hi = ctypes.c_float(), ctypes.c_float()
        self._call("mf_grid_min_max", self.n, self.ptr, ctypes.byref(lo), ctypes.byref(hi), self.parent.stream)
        return lo.value, hi.value

    def getMax(self): return self._minmax()[1]
    def getMin(self): return self._minmax()[0]


class IntGrid(GridBase):
    _kind, _ncomp, _gtype = "int", 1, GridBase.TypeInt
    _cname_py, _cname_cpp, _T = "IntGrid", "Grid", "int"

    def setConst(self, v): self._call("mf_fill_i32", self.n, self.ptr, int(v), self.parent.stream)
    def clear(self): self._call("mf_fill_i32", self.n, self.ptr, 0, self.parent.stream)

    # scene-side conveniences of Grid<int> (grid.cpp:370-380): exact integer reductions on the device tensor
    def _sync(self): self.parent.sync()
    def getMin(self): self._sync(); return float(self.data.min().item())
    def getMax(self): self._sync(); return float(self.data.max().item())
    def getMaxAbs(self): return max(abs(self.getMin()), abs(self.getMax()))
    def sub(self, a): self._check_same(a); self._sync(); self.data.sub_(a.data)
    def add(self, a): self._check_same(a); self._sync(); self.data.add_(a.data)
    def addConst(self, v): self._sync(); self.data.add_(int(v))
    def multConst(self, v): self._sync(); self.data.mul_(int(v))
    def addScaled(self, a, f): self._check_same(a); self._sync(); self.data.add_(a.data * int(f))


class VecGrid(GridBase):
    """Grid<Vec3> (python: VecGrid / Vec3Grid), SoA storage."""
    _kind, _ncomp, _gtype = "vec", 3, GridBase.TypeVec3
    _cname_py, _cname_cpp, _T = "VecGrid", "Grid", "Vec3"

    def setConst(self, v):
        v = _to_vec3(v)
        for c, x in enumerate((v.x, v.y, v.z)):
            self._call("mf_fill_f32", self.n, _ptr(self.data[c * self.n:]), float(x), self.parent.stream)

    def multConst(self, v):
        v = _to_vec3(v)
        for c, x in enumerate((v.x, v.y, v.z)):
            self._call("mf_grid_mult_const", self.n, _ptr(self.data[c * self.n:]), float(x), self.parent.stream)

    def addConst(self, v):
        v = _to_vec3(v)
        for c, x in enumerate((v.x, v.y, v.z)):
            self._call("mf_grid_add_const", self.n, _ptr(self.data[c * self.n:]), float(x), self.parent.stream)

    def addScaled(self, a, f):
        """Grid<Vec3>::addScaled(a, Vec3 factor): me += a * factor, component-wise (grid.cpp:283-285)"""
        self._check_same(a)
        f = _to_vec3(f)
        for c, x in enumerate((f.x, f.y, f.z)):
            self._call("mf_grid_scaled_add", self.n, _ptr(self.data[c * self.n:]), _ptr(a.data[c * a.n:]), float(x), self.parent.stream)

    def add(self, a): self._check_same(a); self._call("mf_grid_add", 3 * self.n, self.ptr, a.ptr, self.parent.stream)
    def sub(self, a): self._check_same(a); self._call("mf_grid_sub", 3 * self.n, self.ptr, a.ptr, self.parent.stream)
    def mult(self, a): self._check_same(a); self._call("mf_grid_mult", 3 * self.n, self.ptr, a.ptr, self.parent.stream)
    def safeDivide(self, a): self._check_same(a); self._call("mf_grid_safe_divide", 3 * self.n, self.ptr, a.ptr, self.parent.stream)

    def stomp(self, th):
        th = _to_vec3(th)
        for c, x in enumerate((th.x, th.y, th.z)):
            self._call("mf_grid_stomp", self.n, _ptr(self.data[c * self.n:]), float(x), self.parent.stream)

    def getMaxAbs(self):
        r = ctypes.c_float()
        self._call("mf_grid_max_abs_vec3", self.n, self.ptr, ctypes.byref(r), self.parent.stream)
        return r.value

    getMax = getMaxAbs

    def getInterpolated(self, pos):
        """Grid<Vec3>::getInterpolated -> interpol<Vec3>, grid.h:150, util/interpol.h:71-82: every component like a Real grid's.
        Host-only: 24 elements are read back."""
        return vec3(*self._interpolated(pos, False))

    def clamp_norm(self, val):
        """Grid<Vec3>::clamp_norm -> knGridClampNorm, grid.cpp:306-317: where the fp32 norm n exceeds val, every component is
        multiplied by the one quotient val / n (include/open/manta_hip_movingobs.h)"""
        lib = _extension_lib(self.parent, "%s::clamp_norm" % type(self)._cname_py, "movingobs")
        lib.call("mf_movingobs_clamp_norm", self.n, 3, self.ptr, float(np.float32(val)), self.parent.stream)

    def getMin(self):
        """sqrt(CompMinVec), grid.cpp:364-366: smallest normSquare (x*x + y*y + z*z in fp32)"""
        self.parent.sync()
        d, n = self.data, self.n
        return float((d[:n] * d[:n] + d[n:2 * n] * d[n:2 * n] + d[2 * n:3 * n] * d[2 * n:3 * n]).min().sqrt().item())

    def setBound(self, value, boundaryWidth=1):
        """Grid<Vec3>::setBound -> knSetBoundary, grid.cpp:629-637"""
        v = _to_vec3(value)
        for c, x in enumerate((v.x, v.y, v.z)):
            self._call("mf_grid_set_bound", self.sx, self.sy, self.sz, _ptr(self.data[c * self.n:]), float(x), int(boundaryWidth), self.parent.stream)


Vec3Grid = VecGrid


class MACGrid(VecGrid):
    _gtype = GridBase.TypeMAC | GridBase.TypeVec3
    _cname_py, _cname_cpp, _T = "MACGrid", "MACGrid", ""

    def _set_bound_mac(self, name, value, boundaryWidth, rule):
        lib = _extension_lib(self.parent, name, "movingobs")
        v = _to_vec3(value)
        lib.call("mf_movingobs_set_bound_mac", self.sx, self.sy, self.sz, self.ptr, float(np.float32(v.x)), float(np.float32(v.y)),
                 float(np.float32(v.z)), int(boundaryWidth), rule, self.parent.stream)

    def setBoundMAC(self, value, boundaryWidth, normalOnly=False):
        """MACGrid::setBoundMAC, grid.cpp:672-692: knSetBoundaryMAC, or with normalOnly knSetBoundaryMACNorm; every component has its
        own band (include/open/manta_hip_movingobs.h)"""
        self._set_bound_mac("MACGrid::setBoundMAC", value, boundaryWidth, 1 if normalOnly else 0)

    def set_bound_MAC2(self, value, boundaryWidth):
        """MACGrid::set_bound_MAC2 -> kn_set_bound_MAC2, grid.cpp:695-715: the walls of the boundary cells"""
        self._set_bound_mac("MACGrid::set_bound_MAC2", value, boundaryWidth, 2)

    # host-only samplers, grid.h:264-267, 460-506: a few elements read back, the reference's expression in fp32 (0.5 * and 0.25 * of an
    # fp32 sum are exact halvings, so the double literals round to the same fp32).  Every element of the stencil must lie in the grid.
    def _stencil(self, what, i, j, k, reach):
        """plane(c, di, dj, dk) -> the fp32 value of component c at (i + di, j + dj, k + dk); reach: the offsets the sampler reads"""
        i, j, k = int(i), int(j), int(k)
        z3 = self.is3D()
        for di, dj, dk in [(0, 0, 0)] + reach:
            if dk and not z3:
                continue
            self._checked_index(what, i + di, j + dj, k + dk)
        self.parent.sync()
        base = i + self.sx * (j + self.sy * k)

        def plane(c, di=0, dj=0, dk=0):
            return np.float32(self.data[c * self.n + base + di + self.sx * (dj + self.sy * dk)].item())
        return plane, z3

    def getInterpolated(self, pos):
        """MACGrid::getInterpolated -> interpolMAC, grid.h:269, util/interpol.h:116-164: each component is sampled on its own faces
        (the index and the weights of its own axis come from pos, the others from pos - 0.5)"""
        return vec3(*self._interpolated(pos, True))

    def getCentered(self, pos):
        """MACGrid::getCentered(Vec3i), grid.h:460-471: the face values averaged to the cell centre"""
        p = _to_vec3(pos, "Vec3i")
        f, z3 = self._stencil("getCentered", p.x, p.y, p.z, [(1, 0, 0), (0, 1, 0), (0, 0, 1)])
        h = np.float32(0.5)
        return vec3(float(h * (f(0) + f(0, 1))), float(h * (f(1) + f(1, 0, 1))), float(h * (f(2) + f(2, 0, 0, 1))) if z3 else 0.0)

    def getAtMACX(self, i, j, k):
        """MACGrid::getAtMACX, grid.h:473-484: the velocity at the x face of the cell"""
        f, z3 = self._stencil("getAtMACX", i, j, k, [(-1, 0, 0), (0, 1, 0), (-1, 1, 0), (0, 0, 1), (-1, 0, 1)])
        q = np.float32(0.25)
        return vec3(float(f(0)), float(q * (f(1) + f(1, -1) + f(1, 0, 1) + f(1, -1, 1))),
                    float(q * (f(2) + f(2, -1) + f(2, 0, 0, 1) + f(2, -1, 0, 1))) if z3 else 0.0)

    def getAtMACY(self, i, j, k):
        """MACGrid::getAtMACY, grid.h:486-496"""
        f, z3 = self._stencil("getAtMACY", i, j, k, [(0, -1, 0), (1, 0, 0), (1, -1, 0), (0, 0, 1), (0, -1, 1)])
        q = np.float32(0.25)
        return vec3(float(q * (f(0) + f(0, 0, -1) + f(0, 1) + f(0, 1, -1))), float(f(1)),
                    float(q * (f(2) + f(2, 0, -1) + f(2, 0, 0, 1) + f(2, 0, -1, 1))) if z3 else 0.0)

    def getAtMACZ(self, i, j, k):
        """MACGrid::getAtMACZ, grid.h:498-506; on a 2-D grid the reference's z stride is 0, so the "k - 1" elements are the cell's own"""
        z3 = self.is3D()
        f, _ = self._stencil("getAtMACZ", i, j, k, [(1, 0, 0), (0, 1, 0)] + ([(0, 0, -1), (1, 0, -1), (0, 1, -1)] if z3 else []))
        q, dk = np.float32(0.25), (-1 if z3 else 0)
        return vec3(float(q * (f(0) + f(0, 0, 0, dk) + f(0, 1) + f(0, 1, 0, dk))), float(q * (f(1) + f(1, 0, 0, dk) + f(1, 0, 1) + f(1, 0, 1, dk))),
                    float(f(2)))


class LevelsetGrid(Grid):
    _gtype = GridBase.TypeLevelset | GridBase.TypeReal
    _cname_py, _cname_cpp, _T = "LevelsetGrid", "LevelsetGrid", ""

    @staticmethod
    def invalidTimeValue(): return -1000.0   # levelset.h:45

    def join(self, o):
        """LevelsetGrid::join -> KnJoin, levelset.cpp:107-111"""
        self._check_same(o)
        self._call("mf_levelset_join", self.n, self.ptr, o.ptr, self.parent.stream)

    def subtract(self, o, flags=None, subtractType=0):
        """LevelsetGrid::subtract -> KnSubtract, levelset.cpp:113-118 (this = -o where o < 0)"""
        self._check_same(o)
        self._call("mf_levelset_subtract", self.n, self.ptr, o.ptr, None if flags is None else flags.ptr,
                   int(subtractType), self.parent.stream)

    def initFromFlags(self, flags, ignoreWalls=False):
        """LevelsetGrid::initFromFlags, levelset.cpp:231-238: -0.5 on fluid cells (and obstacle cells with ignoreWalls), else 0.5"""
        if not isinstance(flags, FlagGrid):
            raise RuntimeError("can't convert argument to FlagGrid*")
        self._check_same(flags)
        lib = self.parent.lib
        if lib.resample:
            self._call("mf_levelset_init_from_flags", self.n, self.ptr, flags.ptr, int(bool(ignoreWalls)), self.parent.stream)
            return
        if lib.backend == "hip":
            raise RuntimeError("initFromFlags: %s lacks the resampling extension (manta_hip_resample.h) -- rebuild the library" % lib.path)
        inside = (flags.data & (TypeFluid | (TypeObstacle if ignoreWalls else 0))) != 0
        self.data.copy_(torch.where(inside, -0.5, 0.5).to(torch.float32))

    _create_mesh_told = False

    def createMesh(self, mesh):
        """LevelsetGrid::createMesh, levelset.cpp:330-415: marching cubes on the device (include/open/manta_hip_mesh.h, DESIGN.md
        section 16) -- classify, count, two scans, one 16-byte read-back of the totals, emit.  On the CPU checker backend and on a
        z-slab solver the call is accepted and the mesh is left as it was."""
        s = self.parent
        lib = s.lib
        if lib.backend != "hip" or tuple(s._slab_window) != (0, 0):
            if not LevelsetGrid._create_mesh_told:
                LevelsetGrid._create_mesh_told = True
                from . import api
                api.mantaMsg("createMesh: not run on %s; the mesh is left as it was"
                             % ("a z-slab solver" if lib.backend == "hip" else "the '%s' backend" % lib.backend), 1)
            return None
        if not isinstance(mesh, Mesh):
            raise RuntimeError("can't convert argument to Mesh")
        if not lib.mesh:
            raise RuntimeError("createMesh: %s lacks the mesh extension (manta_hip_mesh.h) -- rebuild the library" % lib.path)
        if not self.is3D():
            raise RuntimeError("Only 3D grids supported so far")
        mesh.clear()
        need = ctypes.c_int64(0)
        lib.call("mf_mesh_scan_bytes", self.sx, self.sy, self.sz, ctypes.byref(need))
        # scratch from the solver's pool: the two scans, and one grid that holds the 16-bit owned masks followed by the cube bytes
        node_off, tri_off, marks = (s._alloc("int", zero=False) for _ in range(3))
        pooled_tmp = need.value <= 4 * self.n
        tmp = s._alloc("int", zero=False) if pooled_tmp else torch.empty(need.value, dtype=torch.uint8, device=s.device)
        try:
            totals = (ctypes.c_int64 * 2)()
            cube = ctypes.c_void_p(marks.data_ptr() + 2 * self.n)
            lib.call("mf_mesh_create_plan", self.sx, self.sy, self.sz, self.ptr, cube, _ptr(marks), _ptr(node_off), _ptr(tri_off),
                     _ptr(tmp), tmp.numel() * tmp.element_size(), totals, s.stream)
            nn, nt = int(totals[0]), int(totals[1])
            mesh._reserve_nodes(nn, keep=False)
            mesh._reserve_tris(nt, keep=False)
            lib.call("mf_mesh_create_emit", self.sx, self.sy, self.sz, self.ptr, cube, _ptr(marks), _ptr(node_off), _ptr(tri_off), nn, nt,
                     mesh.ncap, _ptr(mesh.pos), _ptr(mesh.normal), _ptr(mesh.nflag), mesh.tcap, _ptr(mesh.tri), _ptr(mesh.tflag), s.stream)
            mesh.nn, mesh.nt = nn, nt
        finally:
            for t in (node_off, tri_off, marks) + ((tmp,) if pooled_tmp else ()):
                s._release("int", t)

    _reinit_keep = None     # tests set a list: each march appends (dir, fmFlags, keys) as numpy copies

    def reinitMarching(self, flags, maxTime=4.0, velTransport=None, ignoreWalls=False, correctOuterLayer=True, obstacleType=TypeObstacle):
        """LevelsetGrid::reinitMarching, levelset.cpp:122-228: the inward march, SetUninitialized, the outward march (which transports
        velTransport), SetUninitialized (include/open/manta_hip_reinit.h).  A march pops its heap on the device
        in rounds of mutually distant cells and is bit-identical to the reference's serial loop; a march that cannot prove that for its
        input, and every march under MF_REINIT_SERIAL=1, runs the literal loop on the host.  One scalar read-back per sub-round and one
        per march; plugins.lastReinitStats() has the counts.  Scratch comes from the solver's pool."""
        s = self.parent
        lib = _extension_lib(s, "LevelsetGrid::reinitMarching", "reinit")
        if not isinstance(flags, FlagGrid):
            raise RuntimeError("can't convert argument to FlagGrid")
        if velTransport is not None and not isinstance(velTransport, MACGrid):
            raise RuntimeError("can't convert argument to MACGrid*")
        self._check_same(flags)
        if velTransport is not None:
            self._check_same(velTransport)
        maxTime = float(np.float32(maxTime))
        serial = 1 if os.environ.get("MF_REINIT_SERIAL", "0") not in ("", "0") else 0
        ints = [s._alloc("int", zero=False) for _ in range(5)]
        reals = [s._alloc("real", zero=False) for _ in range(2)]
        vecs = [s._alloc("vec", zero=False)] if velTransport is not None else []
        fm, lst, sel, epoch, snap_fm = ints
        key, snap_phi = reals
        if s._reinit_ctr is None:
            s._reinit_ctr = torch.zeros(8, dtype=torch.int32, device=s.device)
        stats = {"windows": [0, 0], "subrounds": [0, 0], "pops": [0, 0], "serial": [0, 0], "launches": [0, 0], "readbacks": [0, 0]}
        try:
            out = (ctypes.c_int64 * 6)()
            for q, d in enumerate((-1, 1)):
                lib.call("mf_reinit_march", self.sx, self.sy, self.sz, self.ptr, flags.ptr, None if velTransport is None else velTransport.ptr,
                         _ptr(fm), _ptr(key), _ptr(lst), _ptr(sel), _ptr(epoch), _ptr(snap_phi), _ptr(snap_fm), _ptr(vecs[0]) if vecs else None,
                         _ptr(s._reinit_ctr), maxTime, d, int(bool(ignoreWalls)), int(bool(correctOuterLayer)), int(obstacleType), serial,
                         out, s.stream)
                for name, v in zip(("windows", "subrounds", "pops", "serial", "launches", "readbacks"), out):
                    stats[name][q] = int(v)
                if LevelsetGrid._reinit_keep is not None:
                    LevelsetGrid._reinit_keep.append((d, fm.cpu().numpy().copy(), key.cpu().numpy().copy()))
                val = float(np.float32(-np.float64(np.float32(maxTime)) - 1.)) if d < 0 else float(np.float32(np.float64(np.float32(maxTime)) + 1.))
                lib.call("mf_reinit_set_uninitialized", self.sx, self.sy, self.sz, self.ptr, _ptr(fm), flags.ptr, val, int(bool(ignoreWalls)),
                         int(obstacleType), s.stream)
            from . import plugins
            plugins._reinit_stats = {k: tuple(stats[k]) for k in ("windows", "subrounds", "pops", "serial")}
            plugins._reinit_work = {k: tuple(stats[k]) for k in ("launches", "readbacks")}
        finally:
            for t in ints:
                s._release("int", t)
            for t in reals:
                s._release("real", t)
            for t in vecs:
                s._release("vec", t)


class FlagGrid(IntGrid):
    _gtype = GridBase.TypeFlags | GridBase.TypeInt
    _cname_py, _cname_cpp, _T = "FlagGrid", "FlagGrid", ""
    TypeNone, TypeFluid, TypeObstacle, TypeEmpty, TypeInflow, TypeOutflow, TypeOpen, TypeStick = 0, 1, 2, 4, 8, 16, 32, 64

    def __init__(self, parent, dim=3, show=True, name="", **kw):
        IntGrid.__init__(self, parent, show=show, name=name)

    def _view(self):
        return self.data.view(self.sz, self.sy, self.sx)

    def initDomain(self, boundaryWidth=0, wall="xXyYzZ", open="      ", inflow="      ", outflow="      ", phiWalls=None):
        """FlagGrid::initDomain + initBoundaries, grid.cpp:798-908 (index ops on the device, bit-exact)."""
        types, isset = [0] * 6, [False] * 6
        wall, open, inflow, outflow = (s + "      " for s in (wall, open, inflow, outflow))
        faces = "xXyYzZ"
        for i in range(6):
            for f in range(6 if self.is3D() else 4):
                if isset[f]:
                    continue
                ch = faces[f]
                if open[i] == ch:
                    types[f], isset[f] = TypeOpen, True
                elif inflow[i] == ch:
                    types[f], isset[f] = TypeInflow, True
                elif outflow[i] == ch:
                    types[f], isset[f] = TypeOutflow, True
                elif wall[i] == ch:
                    types[f], isset[f] = TypeObstacle, True
        w = int(boundaryWidth)
        v = self._view()
        v.fill_(TypeEmpty)
        # same overwrite order as initBoundaries: x-, x+, y-, y+, z-, z+
        v[:, :, :w + 1] = types[0]
        v[:, :, max(self.sx - 1 - w, 0):] = types[1]
        v[:, :w + 1, :] = types[2]
        v[:, max(self.sy - 1 - w, 0):, :] = types[3]
        if self.is3D():
            v[:w + 1, :, :] = types[4]
            v[max(self.sz - 1 - w, 0):, :, :] = types[5]
        if phiWalls is not None:
            self._init_phi_walls(phiWalls, w, types, isset, wall)

    def _init_phi_walls(self, phi, w, types, isset, wall):
        # InitMin/MaxXWall etc., grid.cpp:750-796: phi = min(dist - 0.5 - w, phi) for every wall side
        dev = self.data.device
        kk, jj, ii = torch.meshgrid(torch.arange(self.sz, device=dev), torch.arange(self.sy, device=dev),
                                    torch.arange(self.sx, device=dev), indexing="ij")
        p = torch.full((self.sz, self.sy, self.sx), 1000000000.0, dtype=torch.float64, device=dev)
        sides = [(ii - 0.5 - w), (self.sx - ii - 1.5 - w), (jj - 0.5 - w), (self.sy - jj - 1.5 - w),
                 (kk - 0.5 - w), (self.sz - kk - 1.5 - w)]
        for f in range(6 if self.is3D() else 4):
            if types[f] == TypeObstacle:
                p = torch.minimum(p, sides[f].to(torch.float64))
        phi.data.copy_(p.to(torch.float32).reshape(-1))

    def fillGrid(self, type=TypeFluid):
        """grid.cpp:922-927"""
        d = self.data
        keep = (d & (TypeObstacle | TypeInflow | TypeOutflow | TypeOpen)) != 0
        d.copy_(torch.where(keep, d, (d & ~(TypeEmpty | TypeFluid)) | int(type)))

    def updateFromLevelset(self, levelset):
        """grid.cpp:910-920"""
        d, phi = self.data, levelset.data
        upd = ((d & (TypeObstacle | TypeOutflow)) == 0) & (phi > LevelsetGrid.invalidTimeValue())
        newv = (d & ~(TypeEmpty | TypeFluid)) | torch.where(phi <= 0, TypeFluid, TypeEmpty).to(torch.int32)
        d.copy_(torch.where(upd, newv, d))

    def mark_surface(self):
        """FlagGrid::mark_surface, grid.cpp:930-972: TypeSurface is cleared everywhere, then set in the fluid cells that touch
        (26 neighbours, 8 in 2-D) the outside of the grid or a non-fluid cell off the outermost layer.  Prints nothing."""
        lib = _extension_lib(self.parent, "FlagGrid::mark_surface", "movingobs")
        lib.call("mf_movingobs_mark_surface", self.sx, self.sy, self.sz, self.ptr, self.parent.stream)

    def clear_obstacle(self, include_boundary=False):
        """FlagGrid::clear_obstacle, grid.cpp:974-984: obstacle cells become TypeEmpty; the outermost layer only with include_boundary"""
        lib = _extension_lib(self.parent, "FlagGrid::clear_obstacle", "movingobs")
        lib.call("mf_movingobs_clear_obstacle", self.sx, self.sy, self.sz, self.ptr, int(bool(include_boundary)), self.parent.stream)

    def countCells(self, flag, bnd=0, mask=None):
        v = self._view()
        if bnd > 0:
            v = v[(slice(bnd, -bnd) if self.is3D() else slice(None)), bnd:-bnd, bnd:-bnd]
        return int(((v & int(flag)) != 0).sum().item())


RealGrid = Grid


# ---------------------------------------------------------------------------------------------------------
# 4-D grids, grid4d.{h,cpp}: component planes of sx*sy*sz*st words, idx = i + sx*(j + sy*(k + sz*t))
# ---------------------------------------------------------------------------------------------------------
def _to_vec4(v, what="Vec4"):
    if isinstance(v, vec4):
        return v
    if isinstance(v, (tuple, list)) and len(v) == 4:
        return vec4(*v)
    raise RuntimeError("can't convert argument to %s" % what)


def _f32_word(x):
    """the 32-bit word of float(x), as the signed int the ABI's int32_t arguments take"""
    return int(np.array([x], np.float32).view(np.int32)[0])


def _c_int(x):
    """int(Real): the C conversion truncates toward zero"""
    return int(max(-2 ** 31, min(2 ** 31 - 1, int(np.float32(x)))))


class Grid4dBase(PbClass):
    TypeNone, TypeReal, TypeInt, TypeVec3, TypeVec4 = 0, 1, 2, 4, 8
    _cname_py, _cname_cpp = "Grid4dBase", "Grid4dBase"
    _kind, _ncomp, _gtype = None, 1, 0

    def __init__(self, parent, show=True, name="", **kw):
        PbClass.__init__(self, parent, name)
        self.data = None
        if not (parent.is3D() and parent.supports4D()):
            raise RuntimeError("To use 4d grids create a 3d solver with fourthDim>0")
        self.sx, self.sy, self.sz = parent.mGridSize
        self.st = parent.getFourthDim()
        self.n = self.sx * self.sy * self.sz * self.st
        if self.n >= 2 ** 31:
            raise RuntimeError("Grid4d: %d cells do not fit 32-bit cell indices" % self.n)

    def getSizeX(self): return self.sx
    def getSizeY(self): return self.sy
    def getSizeZ(self): return self.sz
    def getSizeT(self): return self.st
    def getSize(self): return vec4(self.sx, self.sy, self.sz, self.st)
    def getDx(self): return float(np.float32(1.0 / float(np.float32(max(self.sx, self.sy, self.sz)))))   # the 4th axis is ignored, grid4d.cpp:63-66
    def getType(self): return self._gtype
    def is3D(self): return True
    def is4D(self): return True
    @property
    def dims(self): return (self.sx, self.sy, self.sz, self.st)


class _TypedArray(PbClass):
    """What Grid4d<T> and ParticleDataImpl<T> share: component planes of one element type in `data`, the int forms of the operators
    and the int and norm reductions (kernels of include/open/manta_hip_grid4d.h, refused where that extension is not), and the
    operators that are one line over _binary / _const.  A subclass gives `_count` (the live elements), `_stride` (the words from one
    component plane to the next), `_who` (the prefix of the refusals) and its own _binary, _const and _value: the float forms differ in
    their launches, and the order of argument conversion, refusal and size check is each method's own."""
    _skips_empty = False        # whether a container without elements launches nothing (after the refusals, before the arguments)

    @property
    def ptr(self): return _ptr(self.data)
    def _plane(self, c): return _ptr(self.data[c * self._stride:])
    def _call(self, fn, *args): return self.parent.lib.call(fn, *args)
    @property
    def _is_int(self): return self._T == "int"

    def _ext(self, what):
        """the library if <class>::<what> can run"""
        return _extension_lib(self.parent, self._who + what, "grid4d")

    @property
    def _launches(self): return not self._skips_empty or self._count > 0

    # the int forms: refused first, then one launch over the live elements
    def _int_binary(self, what, op, a, factor=0):
        self._ext(what)
        if self._launches:
            self._call("mf_grid4d_int_binary", op, self._count, self.ptr, a.ptr, int(factor), self.parent.stream)

    def _int_const(self, what, op, v):
        self._ext(what)
        if self._launches:
            self._call("mf_grid4d_int_const", op, self._count, self.ptr, v, self.parent.stream)

    def _int_clamp(self, lo, hi):
        self._ext("clamp")
        if self._launches:
            self._call("mf_grid4d_int_clamp", self._count, self.ptr, _c_int(lo), _c_int(hi), self.parent.stream)

    def add(self, a): self._binary("add", "mf_grid_add", 0, a)
    def sub(self, a): self._binary("sub", "mf_grid_sub", 1, a)
    def mult(self, a): self._binary("mult", "mf_grid_mult", 2, a)
    def addConst(self, s): self._const("addConst", "mf_grid_add_const", 1, s)
    def multConst(self, s): self._const("multConst", "mf_grid_mult_const", 2, s)

    def _min_max(self, what):
        """(min, max) as Reals: of the values (Real, int) or of the norms (the vector types: sqrt of the extreme normSquare)"""
        f32, scalar = np.float32, self._ncomp == 1
        if self._is_int or not scalar:
            self._ext(what)
        if not self._launches:
            return self._min_max_of_none()
        n = self._count
        lo, hi = (ctypes.c_int32(), ctypes.c_int32()) if self._is_int else (ctypes.c_float(), ctypes.c_float())
        if scalar:
            self._call("mf_grid4d_int_min_max" if self._is_int else "mf_grid_min_max", n, self.ptr, ctypes.byref(lo), ctypes.byref(hi), self.parent.stream)
            return f32(lo.value), f32(hi.value)
        self._call("mf_grid4d_norm_min_max", self._ncomp, n, self._stride, self.ptr, ctypes.byref(lo), ctypes.byref(hi), self.parent.stream)
        return np.sqrt(f32(lo.value)), np.sqrt(f32(hi.value))

    def getMin(self): return float(self._min_max("getMin")[0])
    def getMax(self): return float(self._min_max("getMax")[1])

    def getMaxAbs(self):
        lo, hi = self._min_max("getMaxAbs")
        return float(hi) if self._ncomp > 1 else float(max(abs(lo), abs(hi)))


class Grid4d(_TypedArray, Grid4dBase):
    """Grid4d<T>, one subclass per element type.  The flat float operators run through the core entries (every backend); the
    broadcast forms of the vector types, the int forms, the boundaries and the vector / int reductions are kernels of
    include/open/manta_hip_grid4d.h and are refused where that extension is not (Grid4d::<method>)."""
    _cname_py, _cname_cpp, _who = "Grid4d", "Grid4d", "Grid4d::"

    def __init__(self, parent, show=True, name="", **kw):
        if self._kind is None:
            raise RuntimeError("Grid4d is a template: create a Grid4Real, Grid4Int, Grid4Vec3 or Grid4Vec4")
        Grid4dBase.__init__(self, parent, show, name)
        self._count = self._stride = self.n
        self.data = parent._alloc4(self._kind)      # zeroed: the constructor calls clear(), grid4d.cpp:68

    def __del__(self):
        try:
            if self.data is not None:
                self.parent._release4(self._kind, self.data)
        except Exception:
            pass

    @property
    def _N(self): return self._ncomp * self.n

    def _check_same(self, a):
        if not isinstance(a, Grid4d) or a._kind != self._kind:
            raise RuntimeError("can't convert argument to Grid4d<%s>" % self._T)
        if a.dims != self.dims:
            raise RuntimeError("different Grid4d resolutions [%d,%d,%d,%d] vs [%d,%d,%d,%d]" % (a.dims + self.dims))

    def _value(self, v):
        """a T from Python: four floats (unused ones 0) or one int"""
        if self._kind == "real":
            return (float(v), 0., 0., 0.)
        if self._kind == "int":
            return int(v)
        if self._kind == "vec3":
            v = _to_vec3(v)
            return (v.x, v.y, v.z, 0.)
        return tuple(_to_vec4(v))

    def clear(self):
        if self._is_int:
            self._call("mf_fill_i32", self._N, self.ptr, 0, self.parent.stream)
        else:
            self._call("mf_fill_f32", self._N, self.ptr, 0.0, self.parent.stream)

    def copyFrom(self, a, copyType=True):
        self._check_same(a)
        self._call("mf_copy_f32", self._N, self.ptr, a.ptr, self.parent.stream)     # words are copied; copyType: the type marker is the class's
        return self

    def swap(self, other):
        if not isinstance(other, Grid4d) or other._kind != self._kind or other.dims != self.dims:
            raise RuntimeError("Grid4d::swap(): Grid4d dimensions mismatch.")
        self.data, other.data = other.data, self.data

    def _binary(self, what, entry, op, a, factor=0):
        self._check_same(a)
        if self._is_int:
            self._int_binary(what, op, a, factor)
        else:
            self._call(entry, self._N, self.ptr, a.ptr, self.parent.stream)          # one launch over every component

    def addScaled(self, a, factor):
        """Grid4dScaledAdd<T, T>: me += factor * other with a factor of type T, per component"""
        self._check_same(a)
        f = self._value(factor)
        if self._kind == "real":
            self._call("mf_grid_scaled_add", self.n, self.ptr, a.ptr, f[0], self.parent.stream)
        elif self._is_int:
            self._int_binary("addScaled", 3, a, f)
        else:
            self._ext("addScaled")
            self._call("mf_grid4d_vec_scaled_add", self._ncomp, self.n, self.ptr, a.ptr, f[0], f[1], f[2], f[3], self.parent.stream)

    def _const(self, what, entry, op, v):
        v = self._value(v)
        if self._kind == "real":
            self._call(entry, self.n, self.ptr, v[0], self.parent.stream)
        elif self._is_int:
            if op == 0:
                self._call("mf_fill_i32", self.n, self.ptr, v, self.parent.stream)
            else:
                self._int_const(what, op, v)
        else:
            self._ext(what)
            self._call("mf_grid4d_vec_const", op, self._ncomp, self.n, self.ptr, v[0], v[1], v[2], v[3], self.parent.stream)

    def setConst(self, s): self._const("setConst", "mf_fill_f32", 0, s)

    def clamp(self, min, max):
        """kn4dClamp with T(min), T(max): every component of a vector type against the same pair; int(Real) for Grid4Int"""
        if self._is_int:
            self._int_clamp(min, max)
        else:
            self._call("mf_grid_clamp", self._N, self.ptr, float(min), float(max), self.parent.stream)

    def setBound(self, value, boundaryWidth=1):
        """knSetBnd4d, grid4d.cpp:299-311"""
        v = self._value(value)
        self._ext("setBound")
        w = (v, 0, 0, 0) if self._is_int else tuple(_f32_word(x) for x in v)
        self._call("mf_grid4d_set_bound", self.sx, self.sy, self.sz, self.st, self.ptr, self._ncomp, w[0], w[1], w[2], w[3],
                   int(boundaryWidth), self.parent.stream)

    def setBoundNeumann(self, boundaryWidth=1):
        """knSetBnd4dNeumann, grid4d.cpp:313-346; every axis needs 2 * boundaryWidth + 3 cells (the entry refuses less)"""
        self._ext("setBoundNeumann")
        self._call("mf_grid4d_set_bound_neumann", self.sx, self.sy, self.sz, self.st, self.ptr, self._ncomp, int(boundaryWidth),
                   self.parent.stream)

    # numpy bridge: [t][z][y][x](,[c])
    def to_numpy(self):
        self.parent.sync()
        return _planes_to_elements(self.data.detach().cpu().numpy().reshape(self._ncomp, self.n), self.dims[::-1])

    def from_numpy(self, arr):
        flat = _elements_to_planes(arr, self.dims[::-1], self._ncomp).reshape(-1)
        t = torch.from_numpy(flat.astype(np.int32 if self._is_int else np.float32, copy=False))
        self.data.copy_(t.to(self.data.device))
        return self

    def save(self, name):
        """Grid4d<T>::save, grid4d.cpp:120-132 (.uni, .raw)"""
        return _grid4d_save(self, str(name))

    def load(self, name):
        """Grid4d<T>::load, grid4d.cpp:106-118"""
        return _grid4d_load(self, str(name))

    def printGrid(self, zSlice=-1, tSlice=-1, printIndex=False, bnd=0):
        """Grid4d<T>::printGrid, grid4d.cpp:270-289 (host)"""
        a = self.to_numpy()
        fmt = _format_element(self._is_int, self._ncomp, "%+4.6f")
        out = ["\n"]
        for t in range(bnd, self.st - bnd):
            for k in range(bnd, self.sz - bnd):
                for j in range(bnd, self.sy - bnd):
                    for i in range(bnd, self.sx - bnd):
                        if (zSlice >= 0 and k != zSlice) or (tSlice >= 0 and t != tSlice):
                            continue
                        out.append(" ")
                        if printIndex:
                            out.append("  %d,%d,%d,%d:" % (i, j, k, t))
                        out.append(fmt(a[t, k, j, i]))
                        if i == self.sx - 1 - bnd:
                            out.append("\n")
                            if j == self.sy - 1 - bnd:
                                out.append("\n")
                                if k == self.sz - 1 - bnd:
                                    out.append("\n")
        out.append("\n")
        print("Printing '%s' %s " % (self.name, "".join(out)))


class Grid4Real(Grid4d):
    _kind, _ncomp, _gtype, _T = "real", 1, Grid4dBase.TypeReal, "Real"
    _cname_py = "Grid4Real"


class Grid4Int(Grid4d):
    _kind, _ncomp, _gtype, _T = "int", 1, Grid4dBase.TypeInt, "int"
    _cname_py = "Grid4Int"


class Grid4Vec3(Grid4d):
    _kind, _ncomp, _gtype, _T = "vec3", 3, Grid4dBase.TypeVec3, "Vec3"
    _cname_py = "Grid4Vec3"


class Grid4Vec4(Grid4d):
    _kind, _ncomp, _gtype, _T = "vec4", 4, Grid4dBase.TypeVec4, "Vec4"
    _cname_py = "Grid4Vec4"


# .uni / .raw files of 4-D grids (fileio/iogrids.cpp:624-830): the UniHeader with dimT set, then the elements slice by slice (x fastest,
# the vector types with their components together)
def _grid4d_save(g, name):
    ext = fileio.extension(name)
    if ext not in (".uni", ".raw"):
        raise RuntimeError("file '%s' filetype not supported" % name)
    raw = g.to_numpy().tobytes()
    if ext == ".uni":
        fileio.write(name, raw, fileio.GRID4D, _grid_header(g, g.st))
    else:
        fileio.write(name, raw)
    return 1


def _grid4d_load(g, name):
    ext = fileio.extension(name)
    dt = np.int32 if g._is_int else np.float32
    nbytes = 4 * g._N
    shape = (g.st, g.sz, g.sy, g.sx) + ((g._ncomp,) if g._ncomp > 1 else ())
    if ext == ".raw":
        with fileio.Reader(name) as f:
            raw = f.payload(nbytes)
        if len(raw) != nbytes:
            raise RuntimeError("can't read raw file, stream length does not match, %d vs %d" % (nbytes, len(raw)))
    elif ext == ".uni":
        with fileio.Reader(name) as f:
            ident = f.magic()
            if ident != fileio.GRID4D:        # the reference reports an unknown header at debug level 1 and leaves the grid as it is
                print("Unknown header!")
                return 1
            dx, dy, dz, gtype, etype, bpe, dimt = f.header(ident, "can't read file, no 4d header present")
            if bpe != 4 * g._ncomp:
                raise RuntimeError("4d grid element size doesn't match %d vs %d" % (bpe, 4 * g._ncomp))
            if (dx, dy, dz) != (g.sx, g.sy, g.sz):
                raise RuntimeError("grid dim doesn't match, [%+4.2f,%+4.2f,%+4.2f] vs [%d,%d,%d,%d]" % ((dx, dy, dz) + g.dims))
            if _unify_grid_type(gtype) != _unify_grid_type(g._gtype):
                raise RuntimeError("grid type doesn't match %d vs %d" % (gtype, g._gtype))
            if dimt != g.st:
                raise RuntimeError("grid dim4 doesn't match, %d vs [%d,%d,%d,%d]" % ((dimt,) + g.dims))
            raw = f.payload(nbytes)
            if len(raw) != nbytes:
                raise RuntimeError("can't read file, no / not enough data")
    else:
        raise RuntimeError("file '%s' filetype not supported" % name)
    g.from_numpy(np.frombuffer(raw, dtype=dt).reshape(shape).copy())
    return 1


# ---------------------------------------------------------------------------------------------------------
# particles, particle.{h,cpp}: BasicParticleSystem (pos + flag; the fork's pos0 is not on the hot path)
# ---------------------------------------------------------------------------------------------------------
class ParticleDataImpl(_TypedArray):
    _ncomp, _dtype, _who = 1, torch.float32, "ParticleDataImpl::"
    _skips_empty = True

    def __init__(self, parent, name="", **kw):
        PbClass.__init__(self, parent, name)
        self.sys = None
        self.data = torch.zeros(0, dtype=self._dtype, device=parent.device)
        self.cap = 0      # component stride (== pstride of the ABI)
        self.mpGridSource, self.mGridSourceMAC = None, False     # setSource

    def _attach(self, sys):
        self.sys = sys
        self.resize(sys.np, sys.cap)

    def resize(self, np_, cap=None):
        cap = max(cap if cap is not None else np_, np_)
        if cap != self.cap:
            new = torch.zeros(self._ncomp * cap, dtype=self._dtype, device=self.parent.device)
            keep = min(self.cap, cap)
            for c in range(self._ncomp):
                new[c * cap:c * cap + keep] = self.data[c * self.cap:c * self.cap + keep]
            self.data, self.cap = new, cap

    pyResize = resize

    def setSource(self, grid, isMAC=False):
        """ParticleDataImpl<T>::setSource, particle.cpp:341-346: the grid new particles take their value from (adjustNumber's
        insertion); None: new values are 0"""
        if grid is not None and not isinstance(grid, self._source_type):
            raise RuntimeError("can't convert argument to %s*" % self._source_name)
        if isMAC and not isinstance(grid, MACGrid):
            raise RuntimeError("Given grid is not a valid MAC grid")
        self.mpGridSource, self.mGridSourceMAC = grid, bool(isMAC)
    def size(self): return self.sys.np if self.sys else 0
    def clear(self): self.data.zero_()
    @property
    def _count(self): return self.size()
    @property
    def _stride(self): return self.cap

    def to_numpy(self):
        n = self.size()
        return _planes_to_elements(self.data.detach().cpu().numpy().reshape(self._ncomp, self.cap)[:, :n], (n,))

    def from_numpy(self, arr):
        n = self.size()
        for c, plane in enumerate(_elements_to_planes(arr, (n,), self._ncomp)):
            self.data[c * self.cap:c * self.cap + n] = torch.from_numpy(plane).to(self.data.device, self.data.dtype)
        return self

    def copyFrom(self, o):
        self.data.copy_(o.data)
        return self

    # ---- the arithmetic of ParticleDataImpl<T>, particle.cpp:434-673, over the live slots [0, size): the flat float operators through
    # the core entries on each component plane (every backend), the rest through include/open/manta_hip_grid4d.h (refused elsewhere).
    # An empty channel launches nothing, after the refusals.
    def _check_other(self, a):
        if type(a) is not type(self):
            raise RuntimeError("can't convert argument to ParticleDataImpl<%s>" % self._T)
        if a.size() != self.size():
            raise RuntimeError("different pdata size %d vs %d" % (a.size(), self.size()))

    def _value(self, v):
        if self._is_int:
            return int(v)
        if self._ncomp == 1:
            return (float(v),)
        v = _to_vec3(v)
        return (v.x, v.y, v.z)

    def _binary(self, what, entry, op, a, factor=0):
        self._check_other(a)
        if self._is_int:
            self._int_binary(what, op, a, factor)
        elif self.size():
            for c in range(self._ncomp):              # a launch per plane: the planes are `cap` apart, not `size`
                self._call(entry, self.size(), self._plane(c), a._plane(c), self.parent.stream)

    def safeDiv(self, a): self._binary("safeDiv", "mf_grid_safe_divide", 4, a)

    def addScaled(self, a, factor):
        """knPdataScaledAdd<T, T>: me += factor * other, a factor of type T, per component"""
        f = self._value(factor)
        if self._is_int:
            return self._binary("addScaled", None, 3, a, f)
        self._check_other(a)
        if self.size():
            for c in range(self._ncomp):
                self._call("mf_grid_scaled_add", self.size(), self._plane(c), a._plane(c), f[c], self.parent.stream)

    def _const(self, what, entry, op, v):
        v = self._value(v)
        if self._is_int:
            self._int_const(what, op, v)
        elif self.size():
            for c in range(self._ncomp):
                self._call(entry, self.size(), self._plane(c), v[c], self.parent.stream)

    def clamp(self, vmin, vmax):
        """knPdataClamp with T(vmin), T(vmax): per component for Vec3, int(Real) for int"""
        if self._is_int:
            self._int_clamp(vmin, vmax)
        elif self.size():
            for c in range(self._ncomp):
                self._call("mf_grid_clamp", self.size(), self._plane(c), float(vmin), float(vmax), self.parent.stream)

    def _clamp_side(self, what, side, v):
        self._ext(what)
        w = _c_int(v) if self._is_int else _f32_word(v)
        self._call("mf_grid4d_pdata_clamp_side", side, int(self._is_int), self.size(), self.cap, self._ncomp, self.ptr, w, self.parent.stream)

    def clampMin(self, vmin): self._clamp_side("clampMin", 0, vmin)
    def clampMax(self, vmax): self._clamp_side("clampMax", 1, vmax)

    def setConstRange(self, s, begin, end):
        """ParticleDataImpl::setConstRange: slots [begin, end) of every component plane, as given (the reference does not clamp them;
        past the capacity there is nothing to write)"""
        v = self._value(s)
        b, e = max(0, int(begin)), min(self.cap, int(end))
        if e > b:
            for c in range(self._ncomp):
                self.data[c * self.cap + b:c * self.cap + e] = v if self._is_int else v[c]

    def setConstIntFlag(self, s, t, flag):
        """knPdataSetScalarIntFlag: slots with t[idx] & flag take the value"""
        v = self._value(s)
        if not isinstance(t, PdataInt):
            raise RuntimeError("can't convert argument to ParticleDataImpl<int>")
        self._ext("setConstIntFlag")
        if t.size() != self.size():
            raise RuntimeError("different pdata size %d vs %d" % (t.size(), self.size()))
        w = [v, 0, 0] if self._is_int else [_f32_word(x) for x in v] + [0, 0]
        self._call("mf_grid4d_pdata_set_flag", self.size(), self.cap, self._ncomp, self.ptr, w[0], w[1], w[2], t.ptr, int(flag), self.parent.stream)

    def _min_max_of_none(self):
        """an empty channel gives the reference's start values; for Vec3 (CompPdata_MinVec3 / MaxVec3: the lengths) their roots"""
        big = np.finfo(np.float32).max
        if self._ncomp == 1:
            return big, -big
        with np.errstate(invalid="ignore"):
            return np.sqrt(big), np.sqrt(-big)                  # sqrt(-FLT_MAX): the NaN the host's square root gives

    def _sum(self, what, which, t=None, itype=0):
        if t is not None and not isinstance(t, PdataInt):
            raise RuntimeError("can't convert argument to ParticleDataImpl<int>*")
        self._ext(what)
        if t is not None and t.size() != self.size():
            raise RuntimeError("different pdata size %d vs %d" % (t.size(), self.size()))
        r = (ctypes.c_int32 * 3)()
        self._call("mf_grid4d_pdata_sum", which, int(self._is_int), self._ncomp, self.size(), self.cap, self.ptr, None if t is None else t.ptr,
                   int(itype), r, self.parent.stream)
        w = np.array(list(r), np.int32)
        return w if (self._is_int and which == 0) else w.view(np.float32)

    def sum(self, t=None, itype=0):
        """KnPtsSum: fp64 accumulation in a fixed order, rounded once (include/open/manta_hip_grid4d.h); an int channel's is exact"""
        r = self._sum("sum", 0, t, itype)
        if self._is_int:
            return int(r[0])
        return float(r[0]) if self._ncomp == 1 else vec3(float(r[0]), float(r[1]), float(r[2]))

    def sumSquare(self): return float(self._sum("sumSquare", 1)[0])
    def sumMagnitude(self): return float(self._sum("sumMagnitude", 2)[0])

    def printPdata(self, start=-1, stop=-1, printIndex=False):
        """ParticleDataImpl::printPdata, particle.cpp:619-633 (host)"""
        n = self.size()
        s = min(max(start if start > 0 else 0, 0), n)
        e = min(max(stop if stop > 0 else n, 0), n)
        a, fmt = self.to_numpy(), _format_element(self._is_int, self._ncomp)
        print("".join(("%d: " % i if printIndex else "") + fmt(a[i]) + " \n" for i in range(s, e)))

    # .uni / .raw particle data files, fileio/ioparticles.cpp:225-303: the UniPartHeader + the elements; both extensions name the
    # same format
    def _file_name(self, name, doing):
        name = str(name)
        if fileio.extension(name) not in (".uni", ".raw"):
            raise RuntimeError("particle data '" + name + "' filetype not supported for " + doing)
        return name

    def save(self, name):
        """ParticleDataImpl::save, particle.cpp:391-409"""
        name = self._file_name(name, "saving")
        self.parent.sync()
        fileio.write(name, np.ascontiguousarray(self.to_numpy()).tobytes(), fileio.PDATA, (self.size(),) + self.parent.mGridSize + (1, 4 * self._ncomp))
        return 1

    def load(self, name):
        """ParticleDataImpl::load, particle.cpp:371-389 -> readPdataUni.  The reference resizes the channel to the file's count, away
        from its system; here a channel is as long as its system, and another count is refused with the reader's message."""
        with fileio.Reader(self._file_name(name, "loading"), whole=True) as f:
            ident = f.magic()
            if ident != fileio.PDATA:      # readPdataUni reads nothing then and still answers 1; say so, as the 4-D grid reader does
                print("Unknown header!")
                return 1
            dim, dx, dy, dz, etype, bpe = f.header(ident, "can't read file, no header present")
            raw = f.payload()
        if dim != self.size():
            raise RuntimeError("pdata size doesn't match")
        if bpe != 4 * self._ncomp or etype != 1:
            raise RuntimeError("pdata type doesn't match")
        if len(raw) != bpe * dim:
            raise RuntimeError("can't read uni file, stream length does not match, %d vs %d" % (bpe * dim, len(raw)))
        a = np.frombuffer(raw, np.int32 if self._is_int else np.float32, dim * self._ncomp)
        self.from_numpy(a.reshape((dim, 3) if self._ncomp == 3 else (dim,)).copy())
        return 1


class PdataReal(ParticleDataImpl):
    _cname_py, _cname_cpp, _T = "PdataReal", "ParticleDataImpl", "Real"
    _source_type, _source_name = Grid, "Grid<Real>"
    def setConst(self, v): self.data.fill_(float(v))


class PdataInt(ParticleDataImpl):
    _dtype = torch.int32
    _cname_py, _cname_cpp, _T = "PdataInt", "ParticleDataImpl", "int"

    def setSource(self, grid, isMAC=False):
        raise RuntimeError("PdataInt.setSource: integer source grids are not implemented (no scene uses them)")

    def setConst(self, v): self.data.fill_(int(v))


class PdataVec3(ParticleDataImpl):
    _ncomp = 3
    _cname_py, _cname_cpp, _T = "PdataVec3", "ParticleDataImpl", "Vec3"
    _source_type, _source_name = VecGrid, "Grid<Vec3>"

    def setConst(self, v):
        v = _to_vec3(v)
        for c, x in enumerate((v.x, v.y, v.z)):
            self.data[c * self.cap:(c + 1) * self.cap] = float(x)


class ParticleIndexSystem(PbClass):
    """ParticleSystem<ParticleIndexData> (particle.h:228-240): sourceIndex per slot, filled by gridParticleIndex"""
    _cname_py, _cname_cpp, _T = "ParticleIndexSystem", "ParticleIndexSystem", ""

    def __init__(self, parent, name="", **kw):
        PbClass.__init__(self, parent, name)
        self.data = torch.zeros(0, dtype=torch.int32, device=parent.device)
        self.np = 0

    def size(self): return self.np
    pySize = size

    def to_numpy(self): return self.data[:self.np].detach().cpu().numpy().copy()


_libm = None


def _c_sincos(lib, theta):
    """sinf / cosf of the C library, as `sin(Real)` resolves to in mesh.cpp: the library's host entry, or libm itself where the loaded
    library lacks the mesh extension (the CPU test backend)"""
    global _libm
    if lib.mesh:
        sn, cs = ctypes.c_float(0), ctypes.c_float(0)
        lib.call("mf_mesh_sincos", float(theta), ctypes.byref(sn), ctypes.byref(cs))
        return sn.value, cs.value
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for fn in (_libm.sinf, _libm.cosf):
            fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    return float(_libm.sinf(float(theta))), float(_libm.cosf(float(theta)))


def _vertex_normals(pos, tris):
    """Mesh::computeVertexNormals, mesh.cpp:604-622, on host arrays pos[n][3] float32, tris[t][3]: the three contributions of a
    triangle are `nm * (1.0 / (l * l'))` -- a double factor, each product rounded once -- and are summed into the nodes in fp32 in
    triangle order (ufunc.at adds one index after the other); normalize(), vectorbase.h:421-434, sends NaN to the zero vector"""
    f32, f64 = np.float32, np.float64
    nrm = np.zeros((pos.shape[0], 3), f32)
    with np.errstate(all="ignore"):
        if tris.shape[0]:
            p0, p1, p2 = pos[tris[:, 0]], pos[tris[:, 1]], pos[tris[:, 2]]
            n0, n1, n2 = p0 - p1, p1 - p2, p2 - p0
            l0, l1, l2 = [v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2] for v in (n0, n1, n2)]
            nm = np.stack([n0[:, 1] * n1[:, 2] - n0[:, 2] * n1[:, 1], n0[:, 2] * n1[:, 0] - n0[:, 0] * n1[:, 2],
                           n0[:, 0] * n1[:, 1] - n0[:, 1] * n1[:, 0]], 1)
            w = np.stack([1.0 / (l0 * l2).astype(f64), 1.0 / (l0 * l1).astype(f64), 1.0 / (l1 * l2).astype(f64)], 1)     # [t][corner]
            contrib = (nm.astype(f64)[:, None, :] * w[:, :, None]).astype(f32)
            np.add.at(nrm, tris.reshape(-1), contrib.reshape(-1, 3))
        l = nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] + nrm[:, 2] * nrm[:, 2]
        eps2 = f32(VECTOR_EPSILON) * f32(VECTOR_EPSILON)
        one = np.abs(l.astype(f64) - 1.0) < f64(eps2)
        scaled = ~one & (l > eps2)
        fac = (1.0 / np.sqrt(l.astype(f64)).astype(f32).astype(f64)).astype(f32)
        nrm[scaled] = nrm[scaled] * fac[scaled, None]
        nrm[~one & ~scaled] = 0
    return nrm


def _atoi(s):
    m = re.match(r"\s*[+-]?\d+", s)
    return int(m.group(0)) if m else 0


class Mesh(PbClass):
    """Mesh, mesh.{h,cpp}: a triangle mesh resident on the solver's device.  Nodes are structure-of-arrays -- pos[3][ncap],
    normal[3][ncap], flags[ncap] -- and triangles c[3][tcap] (int32 node numbers) with flags[tcap]; the buffers grow geometrically and
    are reused from call to call.  createMesh (LevelsetGrid), advectInGrid and the node transforms are kernels of
    include/open/manta_hip_mesh.h; save / load are host code.  The corner table and the 1-ring lookup are device tables of
    include/open/manta_hip_meshops.h, cached until the triangle list changes (corners_numpy, ring_numpy).  No Mdata channels."""
    _cname_py, _cname_cpp, _T = "Mesh", "Mesh", ""
    NfNone, NfFixed, NfMarked, NfKillme, NfCollide = 0, 1, 2, 4, 8
    FfNone, FfDoubled, FfMarked = 0, 1, 2
    m_color, m_b2D = vec3(-1, -1, -1), False        # the fork's statics, mesh.cpp:317-318: stored, no effect without a GUI

    def __init__(self, parent, name="", **kw):
        PbClass.__init__(self, parent, name)
        dev = parent.device
        self.nn, self.ncap, self.nt, self.tcap = 0, 0, 0, 0
        self.pos = torch.zeros(0, dtype=torch.float32, device=dev)
        self.normal = torch.zeros(0, dtype=torch.float32, device=dev)
        self.nflag = torch.zeros(0, dtype=torch.int32, device=dev)
        self.tri = torch.zeros(0, dtype=torch.int32, device=dev)
        self.tflag = torch.zeros(0, dtype=torch.int32, device=dev)
        self._saved_pos, self._saved_n = None, 0
        self._sdf_cap, self._sdf_off, self._sdf_stats = 0, None, None      # the source buffers of meshSDF (_sdf_reserve)
        self._sdf_f = torch.zeros(0, dtype=torch.float32, device=dev)
        self._sdf_i = torch.zeros(0, dtype=torch.int32, device=dev)
        self._topo_gen, self._conn, self._conn_gen = 0, None, -1          # the connectivity tables and the generation they are of

    # --- storage ---
    def _reserve_nodes(self, n, keep=True):
        if n <= self.ncap:
            return
        cap, dev = max(n, 2 * self.ncap), self.parent.device
        pos = torch.zeros(3 * cap, dtype=torch.float32, device=dev)
        normal = torch.zeros(3 * cap, dtype=torch.float32, device=dev)
        nflag = torch.zeros(cap, dtype=torch.int32, device=dev)
        if keep and self.nn:
            for c in range(3):
                pos[c * cap:c * cap + self.nn] = self.pos[c * self.ncap:c * self.ncap + self.nn]
                normal[c * cap:c * cap + self.nn] = self.normal[c * self.ncap:c * self.ncap + self.nn]
            nflag[:self.nn] = self.nflag[:self.nn]
        self.pos, self.normal, self.nflag, self.ncap = pos, normal, nflag, cap

    def _reserve_tris(self, n, keep=True):
        if n <= self.tcap:
            return
        cap, dev = max(n, 2 * self.tcap), self.parent.device
        tri = torch.zeros(3 * cap, dtype=torch.int32, device=dev)
        tflag = torch.zeros(cap, dtype=torch.int32, device=dev)
        if keep and self.nt:
            for c in range(3):
                tri[c * cap:c * cap + self.nt] = self.tri[c * self.tcap:c * self.tcap + self.nt]
            tflag[:self.nt] = self.tflag[:self.nt]
        self.tri, self.tflag, self.tcap = tri, tflag, cap

    def _rows(self, t, cap, n):
        """[3][cap] device planes -> host [n][3]"""
        self.parent.sync()
        return np.ascontiguousarray(t.view(3, cap)[:, :n].detach().cpu().numpy().T)

    def numNodes(self): return self.nn
    def numTris(self): return self.nt
    def size(self): return self.nn
    def getSizeSlow(self): return self.nn

    def nodes_numpy(self):
        """-> pos[n][3], normal[n][3], flags[n]"""
        n = self.nn
        if n == 0:
            return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
        return self._rows(self.pos, self.ncap, n), self._rows(self.normal, self.ncap, n), self.nflag[:n].detach().cpu().numpy().copy()

    def tris_numpy(self):
        """-> c[t][3], flags[t]"""
        n = self.nt
        if n == 0:
            return np.zeros((0, 3), np.int32), np.zeros(0, np.int32)
        return self._rows(self.tri, self.tcap, n), self.tflag[:n].detach().cpu().numpy().copy()

    def set_numpy(self, pos, normal=None, flags=None, tris=None, triFlags=None):
        """replace the mesh by host arrays (absent normals and flags are zero, absent triangles none)"""
        pos = np.asarray(pos, np.float32).reshape(-1, 3)
        n = pos.shape[0]
        normal = np.zeros((n, 3), np.float32) if normal is None else np.asarray(normal, np.float32).reshape(-1, 3)
        flags = np.zeros(n, np.int32) if flags is None else np.asarray(flags, np.int32).reshape(-1)
        tris = np.zeros((0, 3), np.int32) if tris is None else np.asarray(tris, np.int32).reshape(-1, 3)
        t = tris.shape[0]
        triFlags = np.zeros(t, np.int32) if triFlags is None else np.asarray(triFlags, np.int32).reshape(-1)
        if normal.shape[0] != n or flags.shape[0] != n or triFlags.shape[0] != t:
            raise RuntimeError("Mesh::set_numpy: array lengths do not match")
        self.nn = self.nt = 0
        self._topo_gen += 1
        self._reserve_nodes(n, keep=False)
        self._reserve_tris(t, keep=False)
        dev = self.parent.device
        for c in range(3):
            self.pos[c * self.ncap:c * self.ncap + n] = torch.from_numpy(np.array(pos[:, c])).to(dev)
            self.normal[c * self.ncap:c * self.ncap + n] = torch.from_numpy(np.array(normal[:, c])).to(dev)
            self.tri[c * self.tcap:c * self.tcap + t] = torch.from_numpy(np.array(tris[:, c])).to(dev)
        self.nflag[:n] = torch.from_numpy(np.array(flags)).to(dev)
        self.tflag[:t] = torch.from_numpy(np.array(triFlags)).to(dev)
        self.nn, self.nt = n, t

    def _set_normals(self, normal):
        dev = self.parent.device
        for c in range(3):
            self.normal[c * self.ncap:c * self.ncap + self.nn] = torch.from_numpy(np.ascontiguousarray(normal[:, c])).to(dev)

    # --- plugins of the reference ---
    def clear(self):
        """Mesh::clear, mesh.cpp:143-160 (the buffers stay)"""
        self.nn = self.nt = 0
        self._topo_gen += 1

    def _not_implemented(self, what, why):
        raise RuntimeError("Mesh::%s: not implemented in mantaflow_amd (%s)" % (what, why))

    def fromShape(self, shape=None, append=False): self._not_implemented("fromShape", "no Shape::generateMesh")
    def computeVelocity(self, oldMesh=None, vel=None): self._not_implemented("computeVelocity", "no mesh velocities")
    # --- mesh -> level set (meshSDF, mesh.cpp:868-1005): include/open/manta_hip_meshsdf.h, DESIGN.md section 17 ---
    def _sdf_lib(self, what):
        """the library if Mesh::<what> can run: refused before anything is looked at (argument checks included) on a backend without the
        extension and on a z-slab solver"""
        s = self.parent
        if s.lib.backend != "hip" or tuple(s._slab_window) != (0, 0):
            self._not_implemented(what, "mesh level sets run on the HIP backend, on whole-domain solvers")
        if not s.lib.meshsdf:
            raise RuntimeError("Mesh::%s: %s lacks the mesh level set extension (manta_hip_meshsdf.h) -- rebuild the library" % (what, s.lib.path))
        return s.lib

    def _sdf_reserve(self, n):
        """the source buffers: pos / normal as emitted and as binned ([3][cap] each) and four int rows of sort scratch; geometric growth"""
        if n > self._sdf_cap:
            cap, dev = max(n, 2 * self._sdf_cap), self.parent.device
            self._sdf_f = torch.empty(12 * cap, dtype=torch.float32, device=dev)
            self._sdf_i = torch.empty(4 * cap, dtype=torch.int32, device=dev)
            self._sdf_cap = cap
        if self._sdf_off is None or self._sdf_off.numel() < max(self.nt, 1):
            self._sdf_off = torch.empty(max(self.tcap, 1), dtype=torch.int64, device=self.parent.device)
        if self._sdf_stats is None:
            self._sdf_stats = torch.zeros(4, dtype=torch.int32, device=self.parent.device)

    def _mesh_sdf(self, lib, who, levelset, sigma, cutoff, flood=True):
        """meshSDF(*this, levelset, sigma, cutoff) as plan, emit, bin, gather, flood; one 8-byte read-back sizes the sources and one int
        per flood round ends the fill.  Scratch grids come from the level set's solver's pool."""
        from . import plugins
        if not isinstance(levelset, LevelsetGrid):
            raise RuntimeError("can't convert argument to LevelsetGrid")
        g = levelset.parent
        if not levelset.is3D() or not self.parent.is3D():
            raise RuntimeError("%s: 3-D grids only" % who)
        if tuple(g._slab_window) != (0, 0):
            raise RuntimeError("%s: not implemented on a z-slab solver" % who)
        if g.device != self.parent.device:
            raise RuntimeError("%s: the level set lives on another device than the mesh" % who)
        sigma, cutoff = float(np.float32(sigma)), float(np.float32(cutoff))
        if not sigma > 0:
            raise RuntimeError("%s: sigma must be positive" % who)
        mark = Mesh._sdf_mark
        sx, sy, sz = levelset.dims
        ms = self.parent.mGridSize
        mult = [np.float32(a) / np.float32(b) for a, b in zip((sx, sy, sz), ms)]        # toVec3(gridRes) / toVec3(gridSize)
        self._sdf_reserve(0)
        st = g.stream
        need = ctypes.c_int64(0)
        lib.call("mf_meshsdf_tmp_bytes", self.nt, 0, levelset.n, ctypes.byref(need))
        grids = [g._alloc("int", zero=False) for _ in range(3)]
        ln, start, occ = grids
        tmp = None
        try:
            def scratch(nbytes):
                nonlocal tmp
                if tmp is None or tmp.numel() * tmp.element_size() < nbytes:
                    if nbytes <= 4 * levelset.n and len(grids) == 3:
                        grids.append(g._alloc("int", zero=False))
                        tmp = grids[3]
                    else:
                        tmp = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
                return tmp
            t = scratch(need.value)
            total = ctypes.c_int64(0)
            if mark: mark("start")
            lib.call("mf_meshsdf_plan", self.nt, self.tcap, _ptr(self.tri), self.nn, self.ncap, _ptr(self.pos), _ptr(self._sdf_off), _ptr(t),
                     t.numel() * t.element_size(), ctypes.byref(total), st)
            nsrc = int(total.value)
            self._sdf_reserve(nsrc)
            cap = self._sdf_cap
            f, ik = self._sdf_f, self._sdf_i
            spos, snrm = _ptr(f), ctypes.c_void_p(f.data_ptr() + 12 * cap) if cap else None
            bpos = ctypes.c_void_p(f.data_ptr() + 24 * cap) if cap else None
            bnrm = ctypes.c_void_p(f.data_ptr() + 36 * cap) if cap else None
            if not cap:
                spos = None
            lib.call("mf_meshsdf_emit", self.nt, self.tcap, _ptr(self.tri), self.nn, self.ncap, _ptr(self.pos), _ptr(self._sdf_off), nsrc,
                     float(mult[0]), float(mult[1]), float(mult[2]), cap, spos, snrm, st)
            if mark: mark("sources")
            lib.call("mf_meshsdf_tmp_bytes", 0, nsrc, levelset.n, ctypes.byref(need))
            t = scratch(need.value)
            lib.call("mf_meshsdf_bin", sx, sy, sz, nsrc, cap, spos, snrm, _ptr(ik) if cap else None, bpos, bnrm, _ptr(ln), _ptr(start), _ptr(occ),
                     _ptr(self._sdf_stats), _ptr(t), t.numel() * t.element_size(), st)
            if mark: mark("binning")
            lib.call("mf_meshsdf_gather", sx, sy, sz, cap, bpos, bnrm, _ptr(ln), _ptr(start), _ptr(occ), sigma, cutoff, levelset.ptr, st)
            if mark: mark("gather")
            out = (ctypes.c_int32 * 2)()
            lib.call("mf_meshsdf_flood", sx, sy, sz, levelset.ptr, sigma, cutoff, 1 if flood else 0, _ptr(self._sdf_stats), out, st)
            if mark: mark("flood")
            plugins._mesh_sdf_stats = {"sources": nsrc, "binned": int(out[1]), "rounds": int(out[0])}
        finally:
            for q in grids:
                g._release("int", q)

    _sdf_mark = None      # tools/meshsdf_time.py sets a callable that is told after which stage the call is

    def computeLevelset(self, levelset=None, sigma=None, cutoff=-1.):
        """Mesh::computeLevelset, mesh.cpp:858-860"""
        lib = self._sdf_lib("computeLevelset")
        self._mesh_sdf(lib, "Mesh::computeLevelset", levelset, sigma, cutoff)

    def getLevelset(self, sigma=None, cutoff=-1.):
        """Mesh::getLevelset, mesh.cpp:862-866: a new level set of the mesh's solver"""
        lib = self._sdf_lib("getLevelset")
        if not self.parent.is3D():
            raise RuntimeError("Mesh::getLevelset: 3-D grids only")
        phi = LevelsetGrid(self.parent)
        self._mesh_sdf(lib, "Mesh::getLevelset", phi, sigma, cutoff)
        return phi

    def applyMeshToGrid(self, grid=None, respectFlags=None, cutoff=-1., meshSigma=2., value=None):
        """Mesh::applyMeshToGrid, mesh.cpp:829-856: meshSDF at the grid's size, then cells with sdf < 0 that are not obstacles of
        respectFlags take `value` (an int, a Real or a Vec3 by the grid's type)"""
        lib = self._sdf_lib("applyMeshToGrid")
        who = "Mesh::applyMeshToGrid"
        if not isinstance(grid, GridBase):
            raise RuntimeError("can't convert argument to GridBase*")
        if respectFlags is not None and not isinstance(respectFlags, FlagGrid):
            raise RuntimeError("can't convert argument to FlagGrid*")
        if not grid.is3D():
            raise RuntimeError("%s: 3-D grids only" % who)
        if respectFlags is not None:
            grid._check_same(respectFlags)
        gt = grid.getType()
        if gt & GridBase.TypeInt:
            kind = 0
        elif gt & GridBase.TypeReal:
            kind = 1
        elif gt & GridBase.TypeVec3:
            kind = 2
        else:
            raise RuntimeError("Shape::applyToGrid(): unknown grid type")
        if value is None:
            raise RuntimeError("Argument 'value' is not defined.")
        iv, v = 0, (0.0, 0.0, 0.0)
        if kind == 0:
            iv = int(value)
        elif kind == 1:
            v = (float(value), 0.0, 0.0)
        else:
            v = tuple(float(x) for x in _to_vec3(value))
        g = grid.parent
        sdf = LevelsetGrid(g)
        self._mesh_sdf(lib, who, sdf, meshSigma, cutoff)
        lib.call("mf_meshsdf_apply", grid.sx, grid.sy, grid.sz, sdf.ptr, None if respectFlags is None else respectFlags.ptr, kind, grid.ptr, iv,
                 v[0], v[1], v[2], g.stream)

    # --- connectivity (mesh.cpp:238-292): include/open/manta_hip_meshops.h, DESIGN.md section 26 ---
    def _meshops_scratch(self, nbytes):
        """-> (tensor of at least nbytes, release): a grid of the solver's pool where one is large enough"""
        s = self.parent
        for kind, size in (("int", 4 * s.ncells), ("vec", 12 * s.ncells)):
            if nbytes <= size:
                t = s._alloc(kind, zero=False)
                return t, lambda: s._release(kind, t)
        return torch.empty(nbytes, dtype=torch.uint8, device=s.device), lambda: None

    def _connectivity(self, lib, who):
        """the corner table and the 1-ring lookup of the triangle list as device tensors, rebuilt only when the topology generation has
        moved (clear, set_numpy, load, createMesh, killSmallComponents).  Refusals -- a triangle with a repeated node, a corner without
        an opposite -- are raised before the cache is touched."""
        from . import plugins
        if self._conn is not None and self._conn_gen == self._topo_gen:
            plugins._meshops_stats.update(singletons=0, multi=self._conn["multi"], rebuilt=False)
            return self._conn
        s, dev = self.parent, self.parent.device
        nt, nn = self.nt, self.nn
        conn = {"opposite": torch.empty(max(3 * nt, 1), dtype=torch.int32, device=dev),
                "nodeOff": torch.empty(nn + 1, dtype=torch.int32, device=dev), "nodes": torch.empty(max(6 * nt, 1), dtype=torch.int32, device=dev),
                "triOff": torch.empty(nn + 1, dtype=torch.int32, device=dev), "tris": torch.empty(max(3 * nt, 1), dtype=torch.int32, device=dev)}
        need = ctypes.c_int64(0)
        lib.call("mf_meshops_tmp_bytes", nt, nn, ctypes.byref(need))
        tmp, release = self._meshops_scratch(need.value)
        try:
            out = (ctypes.c_int32 * 4)()
            lib.call("mf_meshops_build", nt, self.tcap, _ptr(self.tri), nn, _ptr(conn["opposite"]), _ptr(conn["nodeOff"]), _ptr(conn["nodes"]),
                     _ptr(conn["triOff"]), _ptr(conn["tris"]), _ptr(tmp), tmp.numel() * tmp.element_size(), out, s.stream)
        finally:
            release()
        if out[3] >= 0:
            raise RuntimeError("%s: triangle %d names a node outside the mesh's %d nodes" % (who, out[3], nn))
        if out[2] >= 0:
            raise RuntimeError("%s: triangle %d has a repeated node" % (who, out[2]))
        plugins._meshops_stats.update(singletons=int(out[0]), multi=int(out[1]), rebuilt=True)
        if out[0]:
            raise RuntimeError("can't rebuild corners, index without an opposite")
        conn["multi"] = int(out[1])
        self._conn, self._conn_gen = conn, self._topo_gen
        return conn

    def corners_numpy(self):
        """-> opposite[3 * numTris] int32, the corner table of Mesh::rebuildCorners (corner 3t + c is node c of triangle t)"""
        from . import plugins
        lib = plugins._extension_lib(self.parent, "Mesh::corners_numpy", "meshops")
        conn = self._connectivity(lib, "Mesh::corners_numpy")
        self.parent.sync()
        return conn["opposite"][:3 * self.nt].cpu().numpy().copy()

    def ring_numpy(self):
        """-> (nodeOff[n + 1], nodes, triOff[n + 1], tris): the 1-ring lookup of Mesh::rebuildLookup as two CSR tables, ascending per node"""
        from . import plugins
        lib = plugins._extension_lib(self.parent, "Mesh::ring_numpy", "meshops")
        conn = self._connectivity(lib, "Mesh::ring_numpy")
        self.parent.sync()
        node_off, tri_off = conn["nodeOff"].cpu().numpy().copy(), conn["triOff"].cpu().numpy().copy()
        return node_off, conn["nodes"][:int(node_off[-1])].cpu().numpy().copy(), tri_off, conn["tris"][:int(tri_off[-1])].cpu().numpy().copy()

    def create(self, type=None, name="", **kw): self._not_implemented("create", "no Mdata channels")
    def getNodesDataPointer(self): self._not_implemented("getNodesDataPointer", "nodes are structure-of-arrays device buffers")
    def getTrisDataPointer(self): self._not_implemented("getTrisDataPointer", "triangles are structure-of-arrays device buffers")

    @staticmethod
    def set_color(c): Mesh.m_color = _to_vec3(c)
    @staticmethod
    def set_2D(b2D): Mesh.m_b2D = bool(b2D)
    def get_name(self): return self.getName()
    def set_name(self, s): self.setName(s)

    def advectInGrid(self, flags, vel, integrationMode):
        """Mesh::advectInGrid, mesh.cpp:301-315: one kernel, no clamp, no obstacle test, no delete"""
        from . import plugins
        s = self.parent
        lib = plugins._extension_lib(s, "Mesh::advectInGrid", "mesh")
        if not isinstance(flags, FlagGrid):
            raise RuntimeError("can't convert argument to FlagGrid*")
        if not isinstance(vel, MACGrid):
            raise RuntimeError("can't convert argument to MACGrid*")
        if int(integrationMode) not in (0, 1, 2):
            raise RuntimeError("unknown integration type")
        lib.call("mf_mesh_advect", flags.sx, flags.sy, flags.sz, vel.ptr, self.nn, self.ncap, _ptr(self.pos), _ptr(self.nflag), s.getDt(),
                 int(integrationMode), s.stream)

    def _elementwise(self, entry, v, torch_op):
        """pos (op)= v per component: the kernel, or torch on a backend without the extension (the same single fp32 operation)"""
        s = self.parent
        v = _to_vec3(v)
        if self.nn == 0:
            return
        if s.lib.mesh:
            s.lib.call(entry, self.nn, self.ncap, _ptr(self.pos), float(v.x), float(v.y), float(v.z), s.stream)
            return
        if s.lib.backend == "hip":
            raise RuntimeError("Mesh: %s lacks the mesh extension (manta_hip_mesh.h) -- rebuild the library" % s.lib.path)
        for c, x in enumerate(v):
            torch_op(self.pos[c * self.ncap:c * self.ncap + self.nn], float(np.float32(x)))

    def scale(self, s):
        """mesh.cpp:332-336"""
        self._elementwise("mf_mesh_scale", s, lambda t, x: t.mul_(x))

    def offset(self, o):
        """mesh.cpp:338-341"""
        self._elementwise("mf_mesh_offset", o, lambda t, x: t.add_(x))

    def rotate(self, thetas):
        """mesh.cpp:343-373: about x, then y, then z; a zero angle is skipped; sin and cos are the C library's float functions"""
        s = self.parent
        lib = s.lib
        th = _to_vec3(thetas)
        if not lib.mesh and lib.backend == "hip":
            raise RuntimeError("Mesh: %s lacks the mesh extension (manta_hip_mesh.h) -- rebuild the library" % lib.path)
        for theta, (a, b) in zip(th, ((1, 2), (0, 2), (0, 1))):
            theta = float(np.float32(theta))
            if theta == 0.0:
                continue
            sin_t, cos_t = _c_sincos(lib, theta)
            if (a, b) == (0, 2):
                sin_t = -sin_t
            if self.nn == 0:
                continue
            if lib.mesh:
                lib.call("mf_mesh_rotate_pair", self.nn, self.ncap, _ptr(self.pos), a, b, sin_t, cos_t, s.stream)
            else:
                pa, pb = self.pos[a * self.ncap:a * self.ncap + self.nn], self.pos[b * self.ncap:b * self.ncap + self.nn]
                fa, fb = pa.clone(), pb.clone()
                pa.copy_(fa * cos_t - fb * sin_t)      # each product and the difference are single fp32 operations
                pb.copy_(fb * cos_t + fa * sin_t)

    def save_pos(self):
        """mesh.cpp:320-324"""
        self._saved_n = self.nn
        self._saved_pos = self.pos.view(3, self.ncap)[:, :self.nn].clone() if self.nn else None

    def load_pos(self):
        """mesh.cpp:326-330"""
        if self._saved_n != self.nn:
            raise RuntimeError("# of mesh nodes has changed")
        if self.nn:
            self.pos.view(3, self.ncap)[:, :self.nn].copy_(self._saved_pos)

    # --- file I/O, fileio/iomeshes.cpp:125-388 (host) ---
    @staticmethod
    def _extension(name):
        p = name.rfind(".")
        if p < 0:
            raise RuntimeError("file '" + name + "' does not have an extension")
        return name[p:]

    def _unit_cube(self, pos):
        """grid space -> the unit cube around 0, iomeshes.cpp:204-207: pos -= gs * 0.5 ; pos *= dx in fp32"""
        s = self.parent
        half = (np.array(s.mGridSize, np.float32).astype(np.float64) * 0.5).astype(np.float32)
        return (pos - half[None, :]) * np.float32(s.getDx())

    def save(self, name):
        """Mesh::save, mesh.cpp:203-213.  `.bobj.gz` recomputes the vertex normals first, as the reference's writer does; `.obj` does not."""
        ext = self._extension(name)
        if ext not in (".obj", ".gz"):
            raise RuntimeError("file '" + name + "' filetype not supported")
        pos, normal, _ = self.nodes_numpy()
        tris, _ = self.tris_numpy()
        p = self._unit_cube(pos)
        if ext == ".obj":
            out = ["o MantaMesh\n"]
            out += ["v %g %g %g \n" % tuple(v) for v in p.astype(np.float64)]
            out += ["vn %g %g %g \n" % tuple(v) for v in normal.astype(np.float64)]
            out += ["f %d %d %d \n" % tuple(t) for t in tris.astype(np.int64) + 1]
            with open(name, "w") as f:
                f.write("".join(out))
            return
        normal = _vertex_normals(pos, tris)
        if self.nn:
            self._set_normals(normal)
        with gzip.open(name, "wb", compresslevel=1) as f:
            f.write(struct.pack("<i", self.nn) + np.ascontiguousarray(p, "<f4").tobytes())
            f.write(struct.pack("<i", self.nn) + np.ascontiguousarray(normal, "<f4").tobytes())
            f.write(struct.pack("<i", self.nt) + np.ascontiguousarray(tris, "<i4").tobytes())

    def load(self, name, append=False):
        """Mesh::load, mesh.cpp:186-201.  A refused or unreadable file leaves the mesh as it was."""
        ext = self._extension(name)
        if ext == ".gz":
            if append:
                raise RuntimeError("readBobj: append not yet implemented!")
            self._load_bobj(name)
        elif ext == ".obj":
            self._load_obj(name, bool(append))
        else:
            raise RuntimeError("file '" + name + "' filetype not supported")

    def _load_bobj(self, name):
        try:
            with gzip.open(name, "rb") as f:
                raw = f.read()
        except OSError:
            raise RuntimeError("readBobj: unable to open file")
        at = [0]

        def take(dtype, count):
            a = np.frombuffer(raw, dtype, count, at[0])
            at[0] += a.nbytes
            return a
        try:
            n = int(take("<i4", 1)[0])
            pos = take("<f4", 3 * n).reshape(n, 3)
            m = int(take("<i4", 1)[0])
            nrm = take("<f4", 3 * m).reshape(m, 3)
            t = int(take("<i4", 1)[0])
            tris = take("<i4", 3 * t).reshape(t, 3)
        except ValueError:
            raise RuntimeError("readBobj: file '" + name + "' is truncated")
        s = self.parent
        half = (np.array(s.mGridSize, np.float32).astype(np.float64) * 0.5).astype(np.float32)
        pos = pos / np.float32(s.getDx()) + half[None, :]       # back to grid space, iomeshes.cpp:155-156
        normal = np.zeros((n, 3), np.float32)
        normal[:min(n, m)] = nrm[:min(n, m)]
        self.set_numpy(pos, normal, None, tris, None)

    def _load_obj(self, name, append):
        """readObjFile, iomeshes.cpp:282-348: `v` and `f` lines; `vn` values are read into a copy of a node and so dropped -- loaded
        nodes keep the zero normal of Node(); positions are taken as written (the reader does not undo the writer's scaling)"""
        try:
            with open(name) as f:
                lines = f.read().split("\n")
        except OSError:
            raise RuntimeError("can't open file '" + name + "'")
        base = self.nn if append else 0
        verts, faces = [], []
        for line in lines:
            tok = line.split()
            if not tok or tok[0][0] == "#":
                continue
            if tok[0] == "vn":
                if base + len(verts) == 0:
                    raise RuntimeError("invalid amount of nodes")
            elif tok[0] == "v":
                verts.append([np.float32(x) for x in (tok[1:4] + ["0", "0", "0"])[:3]])
            elif tok[0] == "f":
                c = []
                for face in (tok[1:4] + ["", "", ""])[:3]:
                    idx = _atoi(face.split("/")[0]) - 1
                    if idx < 0:
                        raise RuntimeError("invalid face encountered")
                    c.append(idx + base)
                faces.append(c)
        verts = np.array(verts, np.float32).reshape(-1, 3)
        faces = np.array(faces, np.int32).reshape(-1, 3)
        if append and (self.nn or self.nt):
            pos, normal, fl = self.nodes_numpy()
            tris, tfl = self.tris_numpy()
            self.set_numpy(np.concatenate([pos, verts]), np.concatenate([normal, np.zeros_like(verts)]),
                           np.concatenate([fl, np.zeros(len(verts), np.int32)]), np.concatenate([tris, faces]),
                           np.concatenate([tfl, np.zeros(len(faces), np.int32)]))
        else:
            self.set_numpy(verts, None, None, faces, None)


class BasicParticleSystem(PbClass):
    _cname_py, _cname_cpp, _T = "BasicParticleSystem", "BasicParticleSystem", ""

    def __init__(self, parent, name="", **kw):
        PbClass.__init__(self, parent, name)
        dev = parent.device
        self.np, self.cap = 0, 0
        self.pos = torch.zeros(0, dtype=torch.float32, device=dev)     # SoA [3][cap]
        self.flag = torch.zeros(0, dtype=torch.int32, device=dev)
        self.pdata = []
        # ParticleSystem's delete bookkeeping, particle.h:171-173, 423-427: kill() counts mDeletes and, where mAllowCompress,
        # compresses once mDeletes > mDeleteChunk.  Only addParticle, clear and compress change mDeleteChunk; set_positions (the
        # samplers' buffered insertion) leaves both.  BasicParticleSystem's constructor clears mAllowCompress (particle.cpp:134-138),
        # so its kills only count and doCompress() at the end of adjustNumber is the one compress of a call
        self.mDeletes, self.mDeleteChunk, self.mAllowCompress = 0, 0, False

    def create(self, type, name="", **kw):
        """ParticleBase::create, particle.cpp:77-101: new pdata field sized like the system"""
        pd = type(parent=self.parent, name=name)
        self.registerPdata(pd)
        return pd

    def registerPdata(self, pd):
        self.pdata.append(pd)
        pd._attach(self)

    def pySize(self): return self.np
    def size(self): return self.np
    def getSizeSlow(self): return self.np

    def resizeAll(self, n, cap=None):
        cap = max(cap if cap is not None else n, n)
        if cap != self.cap:
            dev = self.parent.device
            newp = torch.zeros(3 * cap, dtype=torch.float32, device=dev)
            newf = torch.zeros(cap, dtype=torch.int32, device=dev)
            keep = min(self.cap, cap)
            for c in range(3):
                newp[c * cap:c * cap + keep] = self.pos[c * self.cap:c * self.cap + keep]
            newf[:keep] = self.flag[:keep]
            self.pos, self.flag, self.cap = newp, newf, cap
        self.np = n
        for pd in self.pdata:
            pd.resize(n, self.cap)

    def clear(self):
        """ParticleSystem::clear, particle.h:408-412"""
        self.mDeleteChunk = self.mDeletes = 0
        self.resizeAll(0)

    def reserve(self, n):
        """capacity for n particles in every array: grows geometrically, never shrinks"""
        if n > self.cap:
            self.resizeAll(self.np, max(n, 2 * self.cap))

    def compress(self, planned=None):
        """ParticleSystem::compress, particle.h:614-633: deleted slots are filled from the tail, every pdata channel moves along.
        planned: (size, holes) of a plan the library holds already (mf_resample_round)"""
        s = self.parent
        if not s.lib.resample:
            raise RuntimeError(_lib.extension("resample").not_implemented("compress", s.lib.backend))
        if planned is None:
            r = (ctypes.c_int64 * 2)()
            s.lib.call("mf_particles_compress_plan", self.np, _ptr(self.flag), r, s.stream)
            planned = (int(r[0]), int(r[1]))
        size, holes = planned
        for ncomp, t, cap in [(3, self.pos, self.cap), (1, self.flag, self.cap)] + [(pd._ncomp, pd.data, pd.cap) for pd in self.pdata]:
            s.lib.call("mf_particles_compress_move", holes, ncomp, cap, _ptr(t), s.stream)
        self.np = size
        self.mDeletes, self.mDeleteChunk = 0, size // 20

    def doCompress(self, bForce=False):
        """particle.h:142-145"""
        if bForce or self.mDeletes > self.mDeleteChunk:
            self.compress()

    # numpy bridge: positions [np][3], flags [np]
    def set_positions(self, arr, flags=None):
        arr = np.asarray(arr, dtype=np.float32).reshape(-1, 3)
        self.resizeAll(arr.shape[0])
        for c in range(3):
            self.pos[c * self.cap:c * self.cap + self.np] = torch.from_numpy(np.ascontiguousarray(arr[:, c])).to(self.pos.device)
        if flags is None:
            self.flag[:self.np] = 0
        else:
            self.flag[:self.np] = torch.from_numpy(np.asarray(flags, dtype=np.int32)).to(self.flag.device)

    def get_positions(self):
        a = self.pos.detach().cpu().numpy()
        return np.stack([a[c * self.cap:c * self.cap + self.np] for c in range(3)], axis=1)

    def get_flags(self): return self.flag[:self.np].detach().cpu().numpy().copy()

    def getPosPdata(self, target): target.data.copy_(self.pos)
    def setPosPdata(self, source): self.pos.copy_(source.data)

    # small host-side completions of the class (particle.h:132-136, particle.cpp:142-160, 238-269)
    def getPos(self, idx):
        idx = int(idx)
        if not 0 <= idx < self.np:
            raise RuntimeError("ParticleBase::checkPartIndex: index %d out of bounds (size %d)" % (idx, self.np))
        return vec3(*[float(self.pos[c * self.cap + idx].item()) for c in range(3)])

    def setPos(self, idx, pos):
        idx, p = int(idx), _to_vec3(pos)
        if not 0 <= idx < self.np:
            raise RuntimeError("ParticleBase::checkPartIndex: index %d out of bounds (size %d)" % (idx, self.np))
        for c, x in enumerate((p.x, p.y, p.z)):
            self.pos[c * self.cap + idx] = x

    def insertBufferedParticles(self, new_pos, new_flags=None):
        """ParticleSystem::insertBufferedParticles, particle.h:637-663: PNEW is cleared everywhere, the buffered positions are appended
        with PNEW (| their flag), every channel grows with its setSource rule (initNewValue) or zero; the delete bookkeeping stays"""
        new_pos = np.asarray(new_pos, np.float32).reshape(-1, 3)
        if self.np:
            self.flag[:self.np] &= ~PNEW
        k = len(new_pos)
        if k == 0:
            return
        old = self.np
        self.reserve(old + k)
        self.resizeAll(old + k, self.cap)
        dev = self.pos.device
        for c in range(3):
            self.pos[c * self.cap + old:c * self.cap + old + k] = torch.from_numpy(np.ascontiguousarray(new_pos[:, c])).to(dev)
        fl = np.full(k, PNEW, np.int32) if new_flags is None else (np.asarray(new_flags, np.int32) | PNEW)
        self.flag[old:old + k] = torch.from_numpy(fl).to(dev)
        # initNewValue (particle.cpp:348-369): zero, or the channel's source grid sampled at the new positions by the entries behind
        # mapGridToParts / mapMACToParts, run on the new slots alone (the planes of positions, flags and channel from slot `old` on)
        lib, st = self.parent.lib, self.parent.stream
        at = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * old)
        for pd in self.pdata:
            for c in range(pd._ncomp):
                pd.data[c * pd.cap + old:c * pd.cap + old + k] = 0
            g = pd.mpGridSource
            if g is None:
                continue
            if pd.mGridSourceMAC:
                lib.call("mf_map_mac_to_parts", g.sx, g.sy, g.sz, g.ptr, k, self.cap, at(self.pos), at(self.flag), at(pd.data), None, 0, st)
            else:
                lib.call("mf_map_grid_to_parts", g.sx, g.sy, g.sz, pd._ncomp, g.ptr, k, self.cap, at(self.pos), at(self.flag), at(pd.data), st)

    def printParts(self, start=-1, stop=-1, printIndex=False):
        """BasicParticleSystem::printParts (host)"""
        n = self.np
        s = min(max(start if start > 0 else 0, 0), n)
        e = min(max(stop if stop > 0 else n, 0), n)
        pos, fl, vec = self.get_positions(), self.get_flags(), _format_element(False, 3)
        print("".join(("%d: " % i if printIndex else "") + "%s %d\n" % (vec(pos[i]), fl[i]) for i in range(s, e)))

    def writeParticlesText(self, name):
        """BasicParticleSystem::writeParticlesText: the header line, then per slot position, flag and the int, Real and Vec3 channels"""
        ints = [p for p in self.pdata if isinstance(p, PdataInt)]
        reals = [p for p in self.pdata if isinstance(p, PdataReal)]
        vecs = [p for p in self.pdata if isinstance(p, PdataVec3)]
        pos, fl, vec = self.get_positions(), self.get_flags(), _format_element(False, 3)
        ch = [(p.to_numpy(), _format_element(p._is_int, p._ncomp)) for p in ints + reals + vecs]
        out = ["%d, pdata: %d (%d,%d,%d) \n" % (self.np, len(self.pdata), len(ints), len(reals), len(vecs))]
        for i in range(self.np):
            out.append("%d: %s , %d. " % (i, vec(pos[i]), fl[i]) + "".join(fmt(a[i]) + " " for a, fmt in ch) + "\n")
        text = "".join(out)
        print("writeParticlesText: %s" % text, end="")
        try:
            with open(name, "w") as f:
                f.write(text)
        except OSError:
            raise RuntimeError("can't open file!")

    def readParticles(self, source):
        """BasicParticleSystem::readParticles: positions and flags of another system, positions scaled to this solver's resolution"""
        if not isinstance(source, BasicParticleSystem):
            raise RuntimeError("can't convert argument to BasicParticleSystem*")
        a, b = source.parent.mGridSize, self.parent.mGridSize
        factor = np.array([np.float32(b[c]) / np.float32(a[c]) for c in range(3)], np.float32)
        self.set_positions(source.get_positions() * factor[None, :] if source.np else np.zeros((0, 3), np.float32), source.get_flags())

    def transformPositions(self, dimOld, dimNew):
        """ParticleSystem::transformPositions, particle.h:449-455: every position times calcGridSizeFactor(dimNew, dimOld), the fp32
        quotient per axis that load and readParticles apply; flags and channels stay.  Host-only: no kernel of ours."""
        a, b = _to_vec3(dimOld, "Vec3i"), _to_vec3(dimNew, "Vec3i")
        if not all(int(o) > 0 for o in (a.x, a.y, a.z)):
            raise RuntimeError("transformPositions: dimOld [%d,%d,%d] has a side that is not positive" % (int(a.x), int(a.y), int(a.z)))
        for c, (o, n) in enumerate(((a.x, b.x), (a.y, b.y), (a.z, b.z))):
            if self.np:
                self.pos[c * self.cap:c * self.cap + self.np] *= float(np.float32(int(n)) / np.float32(int(o)))

    # .uni particle files, fileio/ioparticles.cpp:130-223: the UniPartHeader + [pos.x pos.y pos.z flag] per particle
    _UNI_RECORD = np.dtype([("pos", "<f4", 3), ("flag", "<i4")])

    def save(self, name):
        """BasicParticleSystem::save, particle.cpp:213-236: `.uni` (and `.raw`, the same format)"""
        if fileio.extension(name) not in (".uni", ".raw"):
            raise RuntimeError("particle '" + name + "' filetype not supported for saving")
        rec = np.zeros(self.np, self._UNI_RECORD)
        if self.np:
            rec["pos"], rec["flag"] = self.get_positions(), self.get_flags()
        fileio.write(name, rec.tobytes(), fileio.PARTS, (self.np,) + self.parent.mGridSize + (0, 16))
        return 1

    def load(self, name):
        """BasicParticleSystem::load, particle.cpp:195-211 -> readParticlesUni: every channel is resized, positions are scaled from
        the file's solver resolution to this solver's (transformPositions: an fp32 factor per axis)"""
        if fileio.extension(name) not in (".uni", ".raw"):
            raise RuntimeError("particle '" + name + "' filetype not supported for loading")
        with fileio.Reader(name, whole=True) as f:
            ident = f.magic()
            if ident == fileio.PARTS_V1:
                raise RuntimeError("particle uni file format v01 not supported anymore")
            if ident != fileio.PARTS:
                return 1
            dim, dx, dy, dz, etype, bpe = f.header(ident, "can't read file, no header present")
            raw = f.payload()
        if bpe != 16 or etype != 0:
            raise RuntimeError("particle type doesn't match")
        if len(raw) != 16 * dim:
            raise RuntimeError("can't read uni file, stream length does not match, %d vs %d" % (16 * dim, len(raw)))
        rec = np.frombuffer(raw, self._UNI_RECORD, dim)
        gs = self.parent.mGridSize
        factor = np.array([np.float32(gs[c]) / np.float32((dx, dy, dz)[c]) for c in range(3)], np.float32)
        self.set_positions(rec["pos"] * factor[None, :], np.array(rec["flag"]))
        return 1

    def projectOutOfBnd(self, flags, bnd, plane="xXyYzZ", ptype=None, exclude=0):
        """ParticleSystem::projectOutOfBnd, particle.h:592-604"""
        if self.np == 0:
            return
        axis = sum(1 << i for i, ch in enumerate("xXyYzZ") if ch in plane)
        s = self.parent
        s.lib.call("mf_project_out_of_bnd", flags.sx, flags.sy, flags.sz, self.np, self.cap, _ptr(self.pos), _ptr(self.flag),
                   float(bnd), axis, None if ptype is None else ptype.ptr, int(exclude), s.stream)

    def addParticle(self, pos):
        p = _to_vec3(pos)
        old = self.get_positions()
        fl = self.get_flags()
        self.set_positions(np.concatenate([old, np.array([[p.x, p.y, p.z]], np.float32)]), np.concatenate([fl, [0]]))
        self.mDeleteChunk = self.np // 20     # ParticleSystem::add, particle.h:414-420

    def projectOutside(self, gradient):
        """ParticleSystem::projectOutside -> KnProjectParticles, particle.h:551-578: every active particle inside the grid moves along
        the level-set gradient by -|grad| + 0.1 (1 + r), then every active particle is clamped to [1 + jitter, size - 1 - jitter].
        The reference's serial loop draws from one process-wide stream; here a kernel counts each particle's draws, a scan gives its
        place in the stream, the host draws exactly the total (the one read-back) and a second kernel applies them."""
        s = self.parent
        lib = _extension_lib(s, "BasicParticleSystem::projectOutside", "movingobs")
        if not isinstance(gradient, VecGrid):
            raise RuntimeError("can't convert argument to Grid<Vec3>")
        if self.np == 0:
            return
        need = ctypes.c_int64(0)
        lib.call("mf_movingobs_project_scratch", self.np, ctypes.byref(need))
        offsets = torch.empty(self.np + 1, dtype=torch.int32, device=s.device)
        tmp = torch.empty(int(need.value), dtype=torch.uint8, device=s.device)
        total = ctypes.c_int64(0)
        lib.call("mf_movingobs_project_count", gradient.sx, gradient.sy, gradient.sz, self.np, self.cap, _ptr(self.pos), _ptr(self.flag),
                 _ptr(offsets), _ptr(tmp), int(need.value), ctypes.byref(total), s.stream)
        reals = torch.from_numpy(_movingobs().rs.reals(int(total.value)) if total.value else np.zeros(1, np.float32)).to(s.device)
        lib.call("mf_movingobs_project_apply", gradient.sx, gradient.sy, gradient.sz, self.np, self.cap, _ptr(self.pos), _ptr(self.flag),
                 gradient.ptr, _ptr(offsets), _ptr(reals), s.stream)

    def advectInGrid(self, flags, vel, integrationMode, deleteInObstacle=True, stopInObstacle=True, skipNew=False,
                     ptype=None, exclude=0):
        """ParticleSystem::advectInGrid, particle.h:526-550"""
        s = self.parent
        if self.np == 0:
            return
        scratch = None
        if s.lib.backend != "hip":      # CPU implementations of the ABI need x0/u/uTotal scratch
            scratch = torch.zeros(9 * self.cap, dtype=torch.float32, device=s.device)
        s.lib.call("mf_advect_in_grid", flags.sx, flags.sy, flags.sz, flags.ptr, vel.ptr, self.np, self.cap,
                   _ptr(self.pos), _ptr(self.flag), s.getDt(), int(integrationMode), int(bool(deleteInObstacle)),
                   int(bool(stopInObstacle)), int(bool(skipNew)), None if ptype is None else ptype.ptr, int(exclude),
                   _ptr(scratch), s.stream)


# ---------------------------------------------------------------------------------------------------------
# moving obstacles, movingobs.{h,cpp} (include/open/manta_hip_movingobs.h): the process-wide state
# ---------------------------------------------------------------------------------------------------------
class _MovingObstacleState(object):
    """what the reference keeps per process: MovingObstacle::sIDcnt (movingobs.cpp:24) and KnProjectParticles' `static RandomStream
    rand(3123984)` (particle.h:555) of the BasicParticleSystem instance, which is never reseeded"""

    SEED = 3123984

    def __init__(self):
        from .scene import RandomStream
        self.id_count = 10
        self.rs = RandomStream(self.SEED)


_movingobs_state = None


def _movingobs():
    global _movingobs_state
    if _movingobs_state is None:
        _movingobs_state = _MovingObstacleState()
    return _movingobs_state


def resetMovingObstacleState():
    """put MovingObstacle's ID counter back to 10 and projectOutside's random stream back to its seed, as a fresh process of the
    reference has them (no reference counterpart)"""
    global _movingobs_state
    _movingobs_state = _MovingObstacleState()


# ---------------------------------------------------------------------------------------------------------
# turbulence particles, turbulencepart.{h,cpp} (include/ext/manta_hip_turbulence.h)
# ---------------------------------------------------------------------------------------------------------
class _TurbulenceState(object):
    """what the reference keeps in function statics, one per process: seed()'s `static RandomStream rand(34894231)` (cursor: the
    reals drawn so far) and synthesize()'s `static Real ctime` and `static Vec3 inflow`.  Reals are drawn in blocks and handed out
    one attempt at a time, so the cursor counts exactly three per attempt."""

    SEED = 34894231

    def __init__(self):
        self.seek(0)
        self.ctime = np.float32(0)
        self.inflow = np.zeros(3, np.float32)

    def seek(self, cursor):
        from .scene import RandomStream
        self.rs, self.cursor, self.ahead = RandomStream(self.SEED), 0, np.zeros(0, np.float32)
        while self.cursor < cursor:         # MT19937 has no cheap jump: draw and drop
            self.take(min(cursor - self.cursor, 1 << 20))

    def take(self, n):
        if self.ahead.size < n:
            self.ahead = np.concatenate([self.ahead, self.rs.reals(max(n - self.ahead.size, 3072))])
        r, self.ahead = self.ahead[:n], self.ahead[n:]
        self.cursor += n
        return r


_turbulence_state = _TurbulenceState()


def resetTurbulenceParticleState():
    """restart seed()'s random stream and synthesize()'s clock and inflow offset, as a fresh process of the reference has them (no
    reference counterpart)"""
    global _turbulence_state
    _turbulence_state = _TurbulenceState()


def _set_turbulence_particle_state(cursor, ctime, inflow):
    """test hook: the process-wide state as it is after `cursor` reals, with this clock and inflow offset"""
    _turbulence_state.seek(int(cursor))
    _turbulence_state.ctime = np.float32(ctime)
    _turbulence_state.inflow = np.asarray(inflow, np.float32).reshape(3).copy()


def _hsv2rgb(h, s, v):
    """turbulencepart.cpp:35-55 in fp32; `int i = (int)(h * 6)` truncates, so h = 1 gives i = 6 and `i % 6` case 0"""
    f32 = np.float32
    h, s, v = h.astype(f32), f32(s), f32(v)
    h6 = h * f32(6)
    i = h6.astype(np.int32)                    # truncation toward zero, like the C cast
    f = h6 - i.astype(f32)
    one = f32(1)
    p = np.full(h.shape, v * (one - s), f32)
    q = v * (one - f * s)
    t = v * (one - (one - f) * s)
    vv = np.full(h.shape, v, f32)
    sel = np.fmod(i, 6)                        # C's %: the sign of the dividend; a negative case matches none and leaves (0, 0, 0)
    table = [(vv, t, p), (q, vv, p), (p, vv, t), (p, q, vv), (t, p, vv), (vv, p, q)]
    rgb = np.zeros(h.shape + (3,), f32)
    for case, cols in enumerate(table):
        m = sel == case
        for c in range(3):
            rgb[m, c] = cols[c][m]
    return rgb


class TurbulenceParticleSystem(BasicParticleSystem):
    """TurbulenceParticleSystem, turbulencepart.h:25-48: particles with a colour and two texture coordinates that the wavelet noise
    moves.  Storage is BasicParticleSystem's (SoA pos, flag) with three internal Vec3 channels color, tex0, tex1, so advectInGrid and
    compress() apply as they are: compress() fills deleted slots from the tail and every channel moves along.  seed(),
    resetTexCoords() on an empty system and the process-wide state run on every backend; synthesize() and deleteInObstacle() need
    the turbulence extension and a whole-domain solver."""
    _cname_py, _cname_cpp, _T = "TurbulenceParticleSystem", "TurbulenceParticleSystem", ""

    def __init__(self, parent, noise=None, name="", **kw):
        from .scene import NoiseField
        if not isinstance(noise, NoiseField):
            raise RuntimeError("can't convert argument to WaveletNoiseField*")
        BasicParticleSystem.__init__(self, parent, name)
        self.noise = noise
        self.mAllowCompress = True      # ParticleSystem's default; BasicParticleSystem's constructor is the one that clears it
        self.color, self.tex0, self.tex1 = (self.create(PdataVec3) for _ in range(3))

    def _extension_lib(self, who):
        """_extension_lib for a method: z-slab first, then a backend without the extension"""
        return _extension_lib(self.parent, "TurbulenceParticleSystem::" + who, "turbulence")

    def _append(self, pos, color):
        n0, m = self.np, pos.shape[0]
        self.reserve(n0 + m)
        self.resizeAll(n0 + m, self.cap)
        dev = self.pos.device
        for c in range(3):
            col = torch.from_numpy(np.ascontiguousarray(pos[:, c])).to(dev)
            for t, cap in ((self.pos, self.cap), (self.tex0.data, self.tex0.cap), (self.tex1.data, self.tex1.cap)):
                t[c * cap + n0:c * cap + n0 + m] = col
            self.color.data[c * self.color.cap + n0:c * self.color.cap + n0 + m] = torch.from_numpy(np.ascontiguousarray(color[:, c])).to(dev)
        self.flag[n0:n0 + m] = 0
        for pd in self.pdata:               # addEntry(): every other channel gets a zero entry
            if pd not in (self.color, self.tex0, self.tex1):
                for c in range(pd._ncomp):
                    pd.data[c * pd.cap + n0:c * pd.cap + n0 + m] = 0
        self.mDeleteChunk = self.np // 20   # ParticleSystem::add, particle.h:414-420

    def seed(self, shape, num):
        """turbulencepart.cpp:57-68 (host): rejection sampling in the shape's bounding box with the process-wide stream, three reals
        per attempt, x then y then z; colour from the height inside the box"""
        f32 = np.float32
        if not (hasattr(shape, "getExtent") and hasattr(shape, "getCenter") and hasattr(shape, "_inside")):
            raise RuntimeError("can't convert argument to Shape*")
        num = int(num)
        ext, cen = shape.getExtent(), shape.getCenter()
        sz = np.array([ext.x, ext.y, ext.z], f32)
        p0 = np.array([cen.x, cen.y, cen.z], f32) - sz * f32(0.5)
        st = _turbulence_state
        out = np.zeros((num, 3), f32)
        got = 0
        while got < num:
            want = num - got
            m = max(want + want // 2, 16)
            r = st.take(3 * m).reshape(m, 3)
            p = r * sz + p0
            ok = np.nonzero(shape._inside(p[:, 0], p[:, 1], p[:, 2]))[0]
            if ok.size >= want:             # the attempt that yields the last particle ends the call: hand the rest back
                used = int(ok[want - 1]) + 1
                st.ahead = np.concatenate([r[used:].reshape(-1), st.ahead])
                st.cursor -= 3 * (m - used)
                ok = ok[:want]
            out[got:got + ok.size] = p[ok]
            got += ok.size
        if num <= 0:
            return
        with np.errstate(all="ignore"):
            z = (out[:, 2] - p0[2]) / sz[2]
        self._append(out, _hsv2rgb(z, 0.75, 1.0))

    def resetTexCoords(self, num, inflow):
        """turbulencepart.cpp:70-76: tex0 (num == 0) or tex1 = pos - inflow"""
        v = _to_vec3(inflow)
        if self.np == 0:
            return
        lib = self._extension_lib("resetTexCoords")
        tex = self.tex0 if int(num) == 0 else self.tex1
        lib.call("mf_turbulence_reset_tex", self.np, self.cap, _ptr(self.pos), tex.ptr, float(np.float32(v.x)), float(np.float32(v.y)),
                 float(np.float32(v.z)), self.parent.stream)

    def synthesize(self, flags, k, octaves=2, switchLength=10.0, L0=0.1, scale=1.0, inflowBias=0.0):
        """turbulencepart.cpp:112-131: the host half (process-wide clock and inflow offset, the texture resets) and one kernel with a
        thread per slot"""
        f32 = np.float32
        if not isinstance(flags, FlagGrid):
            raise RuntimeError("can't convert argument to FlagGrid*")
        if not isinstance(k, Grid):
            raise RuntimeError("can't convert argument to Grid<Real>*")
        s = self.parent
        lib = self._extension_lib("synthesize")
        st = _turbulence_state
        bias = _to_vec3(inflowBias)
        dt, sl = f32(s.getDt()), f32(switchLength)
        st.inflow = st.inflow + np.array([bias.x, bias.y, bias.z], f32) * dt
        old_alpha = f32(2.0) * _nmod1(st.ctime / sl)
        st.ctime = f32(st.ctime + dt)
        alpha = f32(2.0) * _nmod1(st.ctime / sl)
        if old_alpha < f32(1.0) and alpha >= f32(1.0):
            self.resetTexCoords(0, vec3(*st.inflow))
        if old_alpha > alpha:
            self.resetTexCoords(1, vec3(*st.inflow))
        alpha = f32(1.0)                    # `alpha = 1.0;` overrides the hat function, as written
        if self.np == 0:
            return
        kmin = f32(1.5 * (0.1 * 0.1))       # 1.5*square(0.1): doubles, rounded into the Real parameter
        lib.call("mf_turbulence_synthesize", k.sx, k.sy, k.sz, k.ptr, _ptr(self.noise._tile), self.noise._params(), self.np, self.cap,
                 _ptr(self.pos), self.tex0.ptr, self.tex1.ptr, float(alpha), float(dt), int(octaves), float(f32(scale)),
                 float(f32(1.0) / f32(L0)), float(kmin), s.stream)

    def deleteInObstacle(self, flags):
        """turbulencepart.cpp:133-138: mark every slot inside an obstacle cell, then compress() -- always, not the chunked
        doCompress().  Every position must lie inside the grid (the reference reads the flag grid unchecked)."""
        if not isinstance(flags, FlagGrid):
            raise RuntimeError("can't convert argument to FlagGrid*")
        s = self.parent
        lib = self._extension_lib("deleteInObstacle")
        lib.call("mf_turbulence_mark_in_obstacle", flags.sx, flags.sy, flags.sz, flags.ptr, self.np, self.cap, _ptr(self.pos), _ptr(self.flag),
                 s.stream)
        self.compress()

    def projectOutside(self, gradient):
        raise RuntimeError("TurbulenceParticleSystem::projectOutside: not implemented (it needs obstacleGradient, i.e. reinitMarching, and "
                           "draws from another process-wide random stream)")

    def channels_to_numpy(self):
        """{pos, color, tex0, tex1, flag} of the live slots"""
        return dict(pos=self.get_positions(), color=self.color.to_numpy(), tex0=self.tex0.to_numpy(), tex1=self.tex1.to_numpy(),
                    flag=self.get_flags())


def _nmod1(a):
    """nmod(a, Real(1.0)), general.h:145: fmod (exact) and one conditional add"""
    c = np.fmod(np.float32(a), np.float32(1.0))
    return np.float32(c + np.float32(1.0)) if c < 0 else np.float32(c)


# ---------------------------------------------------------------------------------------------------------
# vortex particles, vortexpart.{h,cpp} (include/open/manta_hip_vortex.h)
# ---------------------------------------------------------------------------------------------------------
class _VortexSeedStream(object):
    """VPseedK41's `static RandomStream rand(3489572)`, one per process (cursor: the reals drawn so far).  Reals are drawn in blocks;
    peek() shows the next ones and advance() consumes them, so the cursor counts exactly what the reference would have drawn."""

    SEED = 3489572

    def __init__(self):
        from .scene import RandomStream
        self.rs, self.cursor, self.ahead = RandomStream(self.SEED), 0, np.zeros(0, np.float32)

    def peek(self, n):
        if self.ahead.size < n:
            self.ahead = np.concatenate([self.ahead, self.rs.reals(max(n - self.ahead.size, 4096))])
        return self.ahead[:n]

    def advance(self, n):
        self.ahead = self.ahead[n:]
        self.cursor += n


_vortex_seed_stream = _VortexSeedStream()


def resetVortexSeedStream():
    """restart VPseedK41's random stream, as a fresh process of the reference has it (no reference counterpart)"""
    global _vortex_seed_stream
    _vortex_seed_stream = _VortexSeedStream()


def _seek_vortex_seed_stream(cursor):
    """test hook: the process-wide stream as it is after `cursor` reals"""
    resetVortexSeedStream()
    _vortex_seed_stream.peek(int(cursor))
    _vortex_seed_stream.advance(int(cursor))


def _c_pow(name, restype):
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for fn in (_libm.sinf, _libm.cosf):
            fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    fn = getattr(_libm, name)
    fn.restype, fn.argtypes = restype, [restype, restype]
    return fn


def _seed_k41_host(lib, strength, sigma0, sigma1, N, p, dirs):
    """the C library's half of VPseedK41 (powf, pow, normalize) for the accepted cells: the library's host entry, or libm itself where
    the loaded library lacks the vortex extension (the CPU test backend) -> sigma[m], vorticity[m][3]"""
    f32 = np.float32
    m = p.shape[0]
    sig, vort = np.zeros(m, f32), np.zeros((m, 3), f32)
    if m == 0:
        return sig, vort
    p, dirs = np.ascontiguousarray(p, f32), np.ascontiguousarray(dirs, f32)
    if lib.vortex:
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        lib.call("mf_vortex_seed_k41", m, float(strength), float(sigma0), float(sigma1), float(N), P(p), P(dirs), P(sig), P(vort))
        return sig, vort
    powf, powd = _c_pow("powf", ctypes.c_float), _c_pow("pow", ctypes.c_double)
    N, strength = f32(N), f32(strength)
    e1 = float(f32(-float(N) + 1.0))
    s0, s1 = f32(powf(float(f32(sigma0)), e1)), f32(powf(float(f32(sigma1)), e1))
    inv = 1. / (-float(N) + 1.0)
    ex = float(f32(-10. / 6. + float(N) / 2.0))
    eps2 = f32(VECTOR_EPSILON) * f32(VECTOR_EPSILON)
    for q in range(m):
        sg = f32(powd((1.0 - float(p[q])) * float(s0) + float(f32(p[q] * s1)), inv))
        v = dirs[q].copy()
        l = f32(f32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        if abs(float(l) - 1.) < float(eps2):
            pass
        elif l > eps2:
            v = v * f32(1. / float(np.sqrt(l)))
        else:
            v[:] = 0
        sig[q] = sg
        vort[q] = (v * strength) * f32(powf(float(sg), ex))
    return sig, vort


class VortexParticleSystem(BasicParticleSystem):
    """VortexParticleSystem, vortexpart.h:23-41: particles with a vorticity and a core size that move in each other's induced velocity
    (advectSelf) and move the nodes of a Mesh (applyToMesh).  Storage is BasicParticleSystem's (SoA pos, flag) with two internal
    channels, vorticity (Vec3) and sigma (Real), so advectInGrid and compress() apply as they are and the channels move along.  The
    two device methods need the vortex extension and a whole-domain solver; everything else runs on every backend."""
    _cname_py, _cname_cpp, _T = "VortexParticleSystem", "VortexParticleSystem", ""

    def __init__(self, parent, name="", **kw):
        BasicParticleSystem.__init__(self, parent, name)
        self.mAllowCompress = True      # ParticleSystem's default; BasicParticleSystem's constructor is the one that clears it
        self.vorticity, self.sigma = self.create(PdataVec3), self.create(PdataReal)
        self._pos2 = None               # the second position buffer of the stages, kept from call to call

    def _extension_lib(self, who):
        return _extension_lib(self.parent, "VortexParticleSystem::" + who, "vortex")

    def save(self, name):
        raise RuntimeError("VortexParticleSystem::save: not a method of the reference's VortexParticleSystem (BasicParticleSystem only)")

    def load(self, name):
        raise RuntimeError("VortexParticleSystem::load: not a method of the reference's VortexParticleSystem (BasicParticleSystem only)")

    # --- host arrays in and out (the reference has no Python way to add a vortex particle except VPseedK41) ---
    def _write(self, n0, pos, vorticity, sigma, flag):
        m, dev = pos.shape[0], self.pos.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        for c in range(3):
            self.pos[c * self.cap + n0:c * self.cap + n0 + m] = up(pos[:, c])
            self.vorticity.data[c * self.vorticity.cap + n0:c * self.vorticity.cap + n0 + m] = up(vorticity[:, c])
        self.sigma.data[n0:n0 + m] = up(sigma)
        self.flag[n0:n0 + m] = up(flag)
        for pd in self.pdata:               # addEntry(): every other channel gets a zero entry
            if pd is not self.vorticity and pd is not self.sigma:
                for c in range(pd._ncomp):
                    pd.data[c * pd.cap + n0:c * pd.cap + n0 + m] = 0

    def set_numpy(self, pos, vorticity, sigma, flag=None):
        """replace the particles by host arrays pos[n][3], vorticity[n][3], sigma[n], flag[n] (absent: 0)"""
        pos = np.asarray(pos, np.float32).reshape(-1, 3)
        n = pos.shape[0]
        vorticity, sigma = np.asarray(vorticity, np.float32).reshape(-1, 3), np.asarray(sigma, np.float32).reshape(-1)
        flag = np.zeros(n, np.int32) if flag is None else np.asarray(flag, np.int32).reshape(-1)
        if vorticity.shape[0] != n or sigma.shape[0] != n or flag.shape[0] != n:
            raise RuntimeError("VortexParticleSystem::set_numpy: array lengths do not match")
        self.resizeAll(n)
        if n:
            self._write(0, pos, vorticity, sigma, flag)

    def numpy(self):
        """{pos, vorticity, sigma, flag} of the slots"""
        self.parent.sync()
        return dict(pos=self.get_positions().reshape(-1, 3), vorticity=self.vorticity.to_numpy().reshape(-1, 3),
                    sigma=self.sigma.to_numpy().reshape(-1), flag=self.get_flags())

    def _append(self, pos, vorticity, sigma):
        n0, m = self.np, pos.shape[0]
        if m:
            self.reserve(n0 + m)
            self.resizeAll(n0 + m, self.cap)
            self._write(n0, pos, vorticity, sigma, np.zeros(m, np.int32))
        self.mDeleteChunk = self.np // 20   # ParticleSystem::add, particle.h:414-420

    # --- the two device methods ---
    def _scratch(self, nfloats):
        """(tensor, release) of at least nfloats floats: a Vec3 grid of the solver's pool where it is large enough"""
        s = self.parent
        if nfloats <= 3 * s.ncells:
            t = s._alloc("vec", zero=False)
            return t, lambda: s._release("vec", t)
        return torch.empty(nfloats, dtype=torch.float32, device=s.device), lambda: None

    def _integrate(self, lib, tpos, tflag, tmask, nT, tcap, pos2, scale, mode):
        s = self.parent
        need = ctypes.c_int64(0)
        lib.call("mf_vortex_scratch_bytes", self.np, ctypes.byref(need))
        held = [self._scratch(3 * tcap), self._scratch(3 * tcap), self._scratch((need.value + 3) // 4)]
        try:
            (x0, _), (ut, _), (tmp, _) = held
            lib.call("mf_vortex_integrate", nT, tcap, _ptr(tpos), _ptr(tflag), tmask, self.np, self.cap, _ptr(self.pos),
                     _ptr(self.flag), self.vorticity.ptr, self.sigma.ptr, float(np.float32(np.float32(scale) * np.float32(s.getDt()))), mode,
                     _ptr(pos2), _ptr(x0), _ptr(ut), _ptr(tmp), tmp.numel() * 4, s.stream)
        finally:
            for _, release in held:
                release()

    def advectSelf(self, scale=1.0, integrationMode=2):
        """vortexpart.cpp:76-79: the particles move in each other's velocity field; the sources move with the stages"""
        lib = self._extension_lib("advectSelf")
        mode = int(integrationMode)
        if mode not in (0, 1, 2):
            raise RuntimeError("unknown integration type")
        if self.np == 0:
            return
        if self._pos2 is None or self._pos2.numel() != 3 * self.cap:
            self._pos2 = torch.empty(3 * self.cap, dtype=torch.float32, device=self.parent.device)
        self._integrate(lib, self.pos, self.flag, PDELETE, self.np, self.cap, self._pos2, scale, mode)

    def applyToMesh(self, mesh, scale=1.0, integrationMode=2):
        """vortexpart.cpp:81-84: the nodes of the mesh move in the particles' velocity field; the particles stay"""
        lib = self._extension_lib("applyToMesh")
        if not isinstance(mesh, Mesh):
            raise RuntimeError("can't convert argument to Mesh*")
        mode = int(integrationMode)
        if mode not in (0, 1, 2):
            raise RuntimeError("unknown integration type")
        if mesh.parent.device != self.parent.device:
            raise RuntimeError("VortexParticleSystem::applyToMesh: the mesh lives on another device than the particles")
        if mesh.nn == 0:
            return
        pos2, release = self._scratch(3 * mesh.ncap)
        try:
            self._integrate(lib, mesh.pos, mesh.nflag, Mesh.NfFixed, mesh.nn, mesh.ncap, pos2, scale, mode)
        finally:
            release()
