"""The z-slab window promise, entry point by entry point: a kernel called on the planes [lo, hi) of a grid with
mf_set_slab_window(lo, gsz) set gives, on the planes its stencil can vouch for, the bits of the same kernel on the undivided grid.

One table of cases (CASES) and the machinery to run a case on any util.Impl
  (a) undivided, on the global arrays                                   -> run(impl, case, shape, None)
  (b) on the planes [lo, hi) of the same arrays under the window         -> run(impl, case, shape, win)
  (c) on the same planes with NO window set (the control of a case whose result depends on absolute z: it must go wrong)
Particle arrays keep global coordinates.  No process group is needed.

reach: how many planes next to a CUT (never next to a domain wall) a case cannot vouch for.  The numbers are the project's own:
what mantaflow_amd/slab.py demands of the ghost width before it calls the kernel; each case states where its number comes from.

GSZ = 30 planes of 15 x 11 (660 bytes per plane: off the 16-byte grid) or 16 x 12 (aligned); windows: interior [7, 20) (13 planes:
no multiple of 4 nor of the z-column length of the semi-Lagrange kernels), lower wall [0, 12), upper wall [18, 30).  The reaches are
kept <= 4 (|v_z| dt < 1, distances <= 3) so that the interior window keeps at least 5 compared planes."""
import contextlib
import ctypes
import math

import numpy as np
import torch

import util
from util import assert_bitexact

GSZ = 30
SHAPES = {"15x11": (15, 11), "16x12": (16, 12)}
WINDOWS = {"interior-7-20": (7, 20), "lower-wall-0-12": (0, 12), "upper-wall-18-30": (18, 30)}
SRC = (8, 6, 15)                         # the coarse grid of the two-resolution cases (global size)
DT = 1.0
cf = ctypes.c_float
PDELETE = 1 << 10


def trim(lo, hi, r, gsz=GSZ):
    """[lo, hi) minus r planes at every cut; a domain wall is no cut"""
    return lo + (r if lo > 0 else 0), hi - (r if hi < gsz else 0)


def src_window(lo, hi):
    """the window of the coarse source grid for the target planes [lo, hi): the sampled planes +-2 (cubic stencil), and never the
    target's own window"""
    f = SRC[2] / GSZ
    return max(0, int(math.floor(lo * f)) - 3), min(SRC[2], int(math.ceil(hi * f)) + 3)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs (global arrays), one set per plane shape
# ---------------------------------------------------------------------------------------------------------------------------
_inputs = {}
_tile = []


def noise_tile():
    if not _tile:
        t = np.zeros(3 * 128 ** 3, np.float32)
        util.Impl("oracle").lib.call("mf_noise_generate_tile", util.P(t), 13322223, None)
        _tile.append(t)
    return _tile[0]


def inputs(shape):
    if shape in _inputs:
        return _inputs[shape]
    sx, sy = SHAPES[shape]
    sz = GSZ
    g = (sz, sy, sx)
    A = {}
    fl = util.make_flags(sx, sy, sz, 5, empty_top=True)
    fo = util.make_flags(sx, sy, sz, 5, empty_top=True, outflow=True)
    for lo, hi in WINDOWS.values():
        # so that every cut is live for the one-plane stencils: an obstacle just below each lower cut and just above each upper cut
        # with fluid on the other side, and outflow cells in the first / last plane of the window with fluid across the cut
        if lo > 0:
            fl[lo - 1, 3:5, 9:12], fl[lo, 3:5, 9:12] = util.OBS, util.FLUID
            fo[lo - 1, 3:5, 4:8], fo[lo, 3:5, 4:8] = util.FLUID, util.EMPTY | util.OUTFLOW
        if hi < sz:
            fl[hi, 3:5, 9:12], fl[hi - 1, 3:5, 9:12] = util.OBS, util.FLUID
            fo[hi, 3:5, 4:8], fo[hi - 1, 3:5, 4:8] = util.FLUID, util.EMPTY | util.OUTFLOW
    A["flags"], A["flags_out"] = fl, fo
    A["flags_liquid"] = np.where(fl & util.OBS, fl, util.EMPTY).astype(np.int32)      # markFluidCells: particles mark the fluid
    vel = util.smooth_vel(sx, sy, sz, 6, 1.8)                                          # dt max|v| = 1.8
    vel[2] *= np.float32(0.95 / np.abs(vel[2]).max())                                  # |v_z| dt < 1: R = 2
    A["vel"] = vel
    A["R"] = int(math.ceil(float(np.abs(vel[2]).max()) * DT)) + 1                      # slab.required_ghost's R
    A["Rp"] = int(math.ceil(float(np.abs(vel).max()) * DT)) + 2                        # advectInGrid
    assert A["R"] == 2 and A["Rp"] == 4
    A["real"] = util.rand_real(g, 7)
    A["vec"] = util.rand_vel(sx, sy, sz, 8)
    A["vec2"] = util.rand_vel(sx, sy, sz, 9)
    A["vec3"] = util.rand_vel(sx, sy, sz, 10)
    A["vec4"] = util.rand_vel(sx, sy, sz, 11)
    A["real2"], A["real3"], A["real4"] = util.rand_real(g, 12), util.rand_real(g, 13), util.rand_real(g, 14)
    A["phi"] = (util.rand_real(g, 15) * 3).astype(np.float32)
    zz, yy, xx = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    # a tilted wavy surface: the extrapolation layers of extrapolateLsSimple follow it through z
    A["phi_smooth"] = (yy - sy / 2 + 2.0 * np.sin(0.6 * xx + 0.9 * zz) + 0.13).astype(np.float32)
    A["phiObs"] = (util.rand_real(g, 16) * 2).astype(np.float32)
    A["weightgrid"] = np.abs(util.rand_vel(sx, sy, sz, 17)) * (np.random.default_rng(18).random((3,) + g) < 0.3)
    A["weightgrid"] = A["weightgrid"].astype(np.float32)
    rng = np.random.default_rng(19)
    fiso = A["flags_liquid"].copy()
    m = rng.random(g) < 0.3
    m[0] = m[-1] = False; m[:, 0] = m[:, -1] = False; m[:, :, 0] = m[:, :, -1] = False
    fiso[m & (fiso == util.EMPTY)] = util.FLUID
    for c in (7, 12, 18, 20):                 # a pair of fluid cells across every cut, alone otherwise
        fiso[c - 2:c + 2, 2:5, 2:5] = util.EMPTY
        fiso[c - 1:c + 1, 3, 3] = util.FLUID
    A["flags_iso"] = fiso
    pos, pflag, pvel = util.make_particles(fl, 2, 20)
    n = pos.shape[1]
    k = max(n // 40, 8)                       # a few particles outside the grid and near the walls
    pos[:, :k] = rng.uniform(-1.5, 31.5, (3, k)).astype(np.float32)
    A["pos"], A["pflag"], A["pvel"] = pos, pflag, pvel
    # APIC addresses its 8 nodes by FLAT index with no bounds check (apic.cpp:34 "TODO"): a particle outside [1, sx-1) x [1, sy-1)
    # reaches rows of other planes, beyond any z reach.  The APIC cases keep every particle inside (border cells are walls in a scene)
    eps = 1e-3
    A["pos_apic"] = np.stack([np.clip(pos[0], 1, sx - 1 - eps), np.clip(pos[1], 1, sy - 1 - eps), np.clip(pos[2], 0, sz - eps)], 0).astype(np.float32)
    A["ptype"] = rng.choice(np.array([1, 4, 1, 1], np.int32), n).astype(np.int32)
    A["preal"] = np.ascontiguousarray(pvel[0])
    A["cp0"], A["cp1"], A["cp2"] = [rng.normal(0, 0.3, pvel.shape).astype(np.float32) for _ in range(3)]
    # particles over the outflow cells too (resetOutflow)
    npo = 3000
    A["pos_out"] = np.stack([rng.uniform(-0.5, sx + 0.5, npo), rng.uniform(-0.5, sy + 0.5, npo), rng.uniform(-0.5, sz + 0.5, npo)], 0).astype(np.float32)
    A["pflag_out"] = np.where(rng.random(npo) < 0.05, PDELETE, 0).astype(np.int32)
    ssx, ssy, ssz = SRC
    A["src_real"] = util.rand_real((ssz, ssy, ssx), 21)
    A["src_vec"] = util.rand_vel(ssx, ssy, ssz, 22)
    A["src_weight"] = np.abs(util.rand_real((ssz, ssy, ssx), 23))
    zz, yy, xx = np.meshgrid(np.arange(ssz), np.arange(ssy), np.arange(ssx), indexing="ij")
    A["src_uv"] = (np.stack([xx, yy, zz], 0) + 0.5 + util.rand_vel(ssx, ssy, ssz, 24, 0.4)).astype(np.float32)
    A["uv"] = (np.stack(np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")[::-1], 0) + 0.5
               + util.rand_vel(sx, sy, sz, 25, 0.4)).astype(np.float32)
    for v in A.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _inputs[shape] = A
    return A


def cell_z(pos):
    return pos[2].astype(np.int32)          # toVec3i truncation


# ---------------------------------------------------------------------------------------------------------------------------
# one run
# ---------------------------------------------------------------------------------------------------------------------------
class Ctx:
    """what a case's run function sees: the sizes of the grid it is called on, and device copies of its inputs"""

    def __init__(self, impl, A, shape, lo, hi, feed, same_src=False):
        self.impl, self.A = impl, A
        self.sx, self.sy = SHAPES[shape]
        self.lo, self.hi, self.sz = lo, hi, hi - lo
        self.dims = (self.sx, self.sy, self.sz)
        self.slo, self.shi = (0, SRC[2]) if (lo, hi) == (0, GSZ) else src_window(lo, hi)
        self.sgsz = SRC[2]
        if same_src:                        # a weight / uv grid of the target's size lives under the target's window
            self.slo, self.shi, self.sgsz = lo, hi, GSZ
        self.sdims = (SRC[0], SRC[1], self.shi - self.slo)
        self.sel = feed                     # P2G: the particles handed to the call (None: all)
        self.R, self.Rp = A["R"], A["Rp"]

    def g(self, name):
        """planes [lo, hi) of a global grid input (the source window for the coarse grids), a fresh device copy"""
        a = self.A[name]
        lo, hi = (self.slo, self.shi) if name.startswith("src_") else (self.lo, self.hi)
        a = a[:, lo:hi] if a.ndim == 4 else a[lo:hi]
        return self.impl.dev(np.array(a, copy=True))

    def p(self, name):
        a = self.A[name]
        if self.sel is not None:
            a = a[..., self.sel]
        return self.impl.dev(np.array(a, copy=True))

    def n(self, name="pos"):
        return int(self.A[name].shape[-1] if self.sel is None else self.sel.sum())

    def zeros(self, ncomp=1, dtype=np.float32, fill=0):
        return self.impl.dev(np.full((ncomp, self.sz, self.sy, self.sx), fill, dtype))

    def call(self, name, *args):
        return self.impl.call(name, *args)

    def noise_params(self):
        P = np.zeros(20, np.float32)
        P[0:3] = [np.float32(1.0) / np.float32(v) for v in (self.sx, self.sy, GSZ)]        # mGsInv of the whole domain
        P[3:6] = [0.31, 0.62, 0.17]
        P[6] = 0.4
        P[7:10] = 11.0
        P[10:13] = [0.1, 0.2, 0.3]
        P[13], P[14], P[15], P[16], P[17] = 0.75, 1.0, 1, 0, 1
        return (ctypes.c_float * 20)(*[float(v) for v in P])

    def tile(self):
        return self.impl.dev(noise_tile())

    @contextlib.contextmanager
    def package(self, dt=DT):
        """the package's host layer on this implementation: a solver whose grids are this run's planes, with _slab_window set
        (core.SolverLib sets the window per call)"""
        from mantaflow_amd import _lib, core
        if self.impl.which == "oracle":
            _lib.use_library(util.ORACLE_LIB, "cpu")
        else:
            _lib.reset()
            _lib.get()
        try:
            s = core.Solver(gridSize=core.vec3(self.sx, self.sy, self.sz), dim=3)
            s.timestep = dt
            if self.windowed:
                s._slab_window = (self.lo, GSZ)
                s._global_size = (self.sx, self.sy, GSZ)
            yield s
            s.sync()
        finally:
            _lib.reset()


def run(impl, case, shape, win=None, window_set=True):
    """outputs of the case as host arrays: g_* grids [ncomp][sz][sy][sx], p_* particle arrays [ncomp][n], x_* anything else"""
    A = inputs(shape)
    lo, hi = (0, GSZ) if win is None else WINDOWS[win]
    feed = None
    if case.feed is not None and win is not None:
        flo, fhi = trim(lo, hi, case.feed)
        kz = cell_z(A[case.pos])
        feed = ((kz >= flo) | (lo == 0)) & ((kz < fhi) | (hi == GSZ))      # a domain wall is no cut: particles beyond it are the call's too
    c = Ctx(impl, A, shape, lo, hi, feed, case.same_src)
    c.windowed = win is not None and window_set
    cd = impl.lib.cdll
    try:
        if c.windowed:
            assert cd.mf_set_slab_window(lo, GSZ) == 0 and cd.mf_set_slab_window_source(c.slo, c.sgsz) == 0
        out = case.fn(c)
        impl.sync()
    finally:
        cd.mf_set_slab_window(0, 0)
        cd.mf_set_slab_window_source(0, 0)
    res = {}
    for k, t in out.items():
        a = impl.host(t).copy() if isinstance(t, torch.Tensor) else np.asarray(t)
        if k.startswith("g_"):
            a = a.reshape(-1, c.sz, c.sy, c.sx)
        elif k.startswith("p_"):
            a = a.reshape(-1, a.shape[-1])
        res[k] = a
    return res


_cache = {}


def run_cached(impl, case, shape, win=None, window_set=True):
    key = (impl.which, case.name, shape, win, window_set)
    if key not in _cache:
        _cache[key] = run(impl, case, shape, win, window_set)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------
def _split(case, shape, win, und, got, inside):
    """pairs (what, windowed values, undivided values) of the planes / particles inside (or, inside = False, trimmed away from)
    the range the case vouches for; and how many planes / particles that is"""
    lo, hi = WINDOWS[win]
    tlo, thi = trim(lo, hi, case.reach)
    A = inputs(shape)
    pairs, planes, parts = [], 0, 0
    for k in und:
        if k.startswith("g_"):
            if inside:
                pairs.append((k, got[k][:, tlo - lo:thi - lo], und[k][:, tlo:thi]))
                planes = thi - tlo
            else:
                ks = [z for z in range(lo, hi) if not tlo <= z < thi]
                pairs.append((k, got[k][:, [z - lo for z in ks]], und[k][:, ks]))
        elif k.startswith("p_"):
            kz = cell_z(A[case.pos])
            sel = (kz >= tlo) & (kz < thi) if inside else ((kz >= lo) & (kz < hi) & ~((kz >= tlo) & (kz < thi)))
            pairs.append((k, got[k][:, sel], und[k][:, sel]))
            parts = int(sel.sum())
    return pairs, planes, parts


def check_window(case, shape, win, und, got, what):
    """windowed against undivided on what is left after trimming the reach at every cut"""
    if case.check is not None:
        return case.check(case, shape, win, und, got, what)
    pairs, planes, parts = _split(case, shape, win, und, got, True)
    assert pairs and (planes >= 4 or parts >= 200), (what, planes, parts)
    for k, a, b in pairs:
        assert_bitexact(a, b, "%s %s (windowed vs undivided)" % (what, k))


def differs(case, shape, win, und, got, inside):
    return any(not np.array_equal(util.bits(a), util.bits(b)) for _, a, b in _split(case, shape, win, und, got, inside)[0])


def check_whole(a, b, what):
    """two implementations under the same window: every output, ghost planes and out-of-window particles included"""
    assert set(a) == set(b)
    for k in a:
        assert_bitexact(a[k], b[k], "%s %s (whole local result)" % (what, k))


def check_gpi(case, shape, win, und, got, what):
    """for every window cell the particle list isys[index[c]:index[c+1]] equals the undivided one (slot numbers differ by an offset)"""
    lo, hi = WINDOWS[win]

    def lists(r, k0, k1):
        idx, isys = r["g_index"][0].reshape(-1), r["x_isys"]
        XY = idx.size // r["g_index"].shape[1]
        end = np.append(idx[1:], len(isys))
        return [tuple(isys[idx[c]:end[c]]) for c in range(k0 * XY, k1 * XY)]
    a, b = lists(got, 0, hi - lo), lists(und, lo, hi)
    assert hi - lo >= 4 and sum(len(x) for x in b) >= 200
    bad = [c for c in range(len(a)) if a[c] != b[c]]
    assert not bad, "%s: particle lists of %d window cells differ, first cell %d: %s vs %s" % (what, len(bad), bad[0], a[bad[0]], b[bad[0]])


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, fn, reach, why, absz=False, pos="pos", feed=None, check=None, sides=("lo", "hi"), same_src=False):
        """sides: the cuts at which the reach is live ("lo": the stencil reads below, "hi": above)"""
        self.name, self.fn, self.reach, self.why, self.absz, self.pos, self.feed, self.check = name, fn, reach, why, absz, pos, feed, check
        self.sides, self.same_src = sides, same_src


CASES = []


def case(name, reach, why, **kw):
    def deco(fn):
        CASES.append(Case(name, fn, reach, why, **kw))
        return fn
    return deco


R = 2       # slab.required_ghost's R = ceil(max|v_z| dt) + 1 for the velocity of inputs() (asserted there)
RP = 4      # ceil(max|v| dt) + 2


# ---- advection --------------------------------------------------------------------------------------------------------------
def _semi_lagrange(kind, ot, osp):
    def fn(c):
        src = c.g({"real": "real", "vec3": "vec", "mac": "vel"}[kind])
        dst = c.zeros(1 if kind == "real" else 3, fill=7)
        c.call("mf_semi_lagrange_" + kind, *c.dims, c.g("vel"), dst, src, DT, ot, osp, None)
        return {"g_dst": dst}
    return fn


for _kind in ("real", "vec3", "mac"):
    for _ot in (1, 2):
        for _os in (1, 2):
            CASES.append(Case("semi_lagrange_%s-trace%d-space%d" % (_kind, _ot, _os), _semi_lagrange(_kind, _ot, _os), R + (_os == 2),
                              "R: trace of max|v_z| dt plus the trilinear gather (slab.required_ghost); cubic: one more, interpol_cubic reads z1-1 .. z1+2"))


def _mc_clamp(mac, ncomp, mode, correct):
    def fn(c):
        f = {1: ("real", "real2", "real3", "real4"), 3: ("vec", "vec2", "vec3", "vec4")}[ncomp]
        orig, fwd, bwd = c.g(f[1]), c.g(f[2]), c.g(f[3])
        nc = () if mac else (ncomp,)
        sfx = "_mac" if mac else ""
        if correct:
            dst = c.zeros(ncomp, fill=7)
            c.call("mf_maccormack_correct_clamp" + sfx, *c.dims, *nc, c.g("flags"), c.g("vel"), dst, orig, fwd, bwd, 0.8, DT, mode, None)
        else:
            dst = c.g(f[0])
            c.call("mf_maccormack_clamp" + sfx, *c.dims, *nc, c.g("flags"), c.g("vel"), dst, orig, fwd, DT, mode, None)
        return {"g_dst": dst}
    return fn


for _mode in (1, 2):
    for _correct in (False, True):
        for _mac, _nc in ((False, 1), (False, 3), (True, 3)):
            CASES.append(Case("maccormack_%sclamp%s-ncomp%d-mode%d" % ("correct_" if _correct else "", "_mac" if _mac else "", _nc, _mode),
                              _mc_clamp(_mac, _nc, _mode, _correct), R, "R: the clamp traces back and forth by max|v_z| dt and reads the 8 cells around (slab.required_ghost)"))


@case("maccormack_correct-ncomp1", 0, "cell-local (KERNEL(idx))")
def _(c):
    dst = c.zeros(1, fill=7)
    c.call("mf_maccormack_correct", *c.dims, 1, c.g("flags"), dst, c.g("real2"), c.g("real3"), c.g("real4"), 0.8, None)
    return {"g_dst": dst}


@case("maccormack_correct-ncomp3", 0, "cell-local (KERNEL(idx))")
def _(c):
    dst = c.zeros(3, fill=7)
    c.call("mf_maccormack_correct", *c.dims, 3, c.g("flags"), dst, c.g("vec2"), c.g("vec3"), c.g("vec4"), 0.8, None)
    return {"g_dst": dst}


@case("maccormack_correct_mac", 1, "reads the flags of the lower neighbour of each face", sides=("lo",))
def _(c):
    dst = c.zeros(3, fill=7)
    c.call("mf_maccormack_correct_mac", *c.dims, c.g("flags"), dst, c.g("vec2"), c.g("vec3"), c.g("vec4"), 0.8, None)
    return {"g_dst": dst}


def _pkg_advect(kind):
    def fn(c):
        from mantaflow_amd import core, plugins
        import cases
        with c.package() as s:
            fl, v = cases.soa_to_grid(core.FlagGrid(s), c.g("flags").cpu().numpy()), cases.soa_to_grid(core.MACGrid(s), c.g("vel").cpu().numpy())
            G, name = {0: (core.Grid, "real"), 2: (core.MACGrid, "vel")}[kind]
            g = cases.soa_to_grid(G(s), c.g(name).cpu().numpy())
            plugins.advectSemiLagrange(fl, v, g, order=2, strength=0.8, clampMode=2)
            s.sync()
            return {"g_dst": g.data.detach().cpu().numpy().copy()}
    return fn


CASES.append(Case("plugins.advectSemiLagrange-order2-real", _pkg_advect(0), 2 * R, "2R: forward and backward pass (slab.required_ghost = 2R)"))
CASES.append(Case("plugins.advectSemiLagrange-order2-mac", _pkg_advect(2), 2 * R, "2R: forward and backward pass (slab.required_ghost = 2R)"))


@case("apply_outflow_bc", 2, "reads the advected velocity two cells around an outflow cell (slab.advectSemiLagrange exchanges 2 planes)")
def _(c):
    vel = c.g("vel")
    c.call("mf_apply_outflow_bc", *c.dims, c.g("flags_out"), vel, c.g("vec"), c.zeros(3), DT, None)
    return {"g_vel": vel}


# ---- grid glue and surface ----------------------------------------------------------------------------------------------------
@case("set_wall_bcs", 1, "flags of the lower neighbour of each face", sides=("lo",))
def _(c):
    vel = c.g("vec")
    c.call("mf_set_wall_bcs", *c.dims, c.g("flags"), vel, None, None)
    return {"g_vel": vel}


@case("set_wall_bcs-obvel", 1, "flags of the lower neighbour of each face", sides=("lo",))
def _(c):
    vel = c.g("vec")
    c.call("mf_set_wall_bcs", *c.dims, c.g("flags"), vel, c.g("vec2"), None)
    return {"g_vel": vel}


@case("add_buoyancy", 1, "density and flags of the lower neighbour of each face", sides=("lo",))
def _(c):
    vel = c.g("vec")
    c.call("mf_add_buoyancy", *c.dims, c.g("flags"), c.g("real"), vel, 0.1, -0.7, 0.3, None)
    return {"g_vel": vel}


def _apply_force(additive, excl):
    def fn(c):
        vel = c.g("vec")
        c.call("mf_apply_force", *c.dims, c.g("flags"), vel, 0.1, -0.7, 0.3, c.g("real") if excl else None, additive, None)
        return {"g_vel": vel}
    return fn


CASES.append(Case("apply_force-additive", _apply_force(1, False), 1, "flags of the lower neighbour of each face", sides=("lo",)))
CASES.append(Case("apply_force-set-exclude", _apply_force(0, True), 1, "flags of the lower neighbour of each face", sides=("lo",)))


@case("mark_isolated_fluid_cell", 1, "flags of the six neighbours")
def _(c):
    fl = c.g("flags_iso")
    c.call("mf_mark_isolated_fluid_cell", *c.dims, fl, util.EMPTY, None)
    return {"g_flags": fl}


@case("compute_energy", 1, "GetCentered reads the faces at i+1, j+1, k+1 (commonkernels.h:126-131): one plane above, none below", sides=("hi",))
def _(c):
    e = c.zeros(1, fill=7)
    c.call("mf_compute_energy", *c.dims, c.g("flags"), c.g("vel"), e, None)
    return {"g_energy": e}


def _extrap_mac_simple(dist, into):
    def fn(c):
        vel = c.g("vec")
        c.call("mf_extrapolate_mac_simple", *c.dims, c.g("flags"), vel, dist, into, c.zeros(1, np.int32), c.zeros(3), None)
        return {"g_vel": vel}
    return fn


CASES.append(Case("extrapolate_mac_simple-d3", _extrap_mac_simple(3, 0), 4, "d + 1: d layers, each one cell further, plus the marking pass"))
CASES.append(Case("extrapolate_mac_simple-d3-intoObs", _extrap_mac_simple(3, 1), 4, "d + 1"))


@case("extrapolate_mac_from_weight-d2", 3, "d + 1")
def _(c):
    vel, w = c.g("vec"), c.g("weightgrid")
    c.call("mf_extrapolate_mac_from_weight", *c.dims, vel, w, 2, None)
    return {"g_vel": vel}


def _extrap_ls(dist, inside, walls):
    def fn(c):
        phi = c.g("phi_smooth")
        c.call("mf_extrapolate_ls_simple", *c.dims, phi, dist, inside, walls, c.zeros(1, np.int32), None)
        return {"g_phi": phi}
    return fn


CASES.append(Case("extrapolate_ls_simple-d2-outside", _extrap_ls(2, 0, 0), 4, "d + 2: first layer, d - 1 passes, the fill of the rest"))
CASES.append(Case("extrapolate_ls_simple-d2-inside", _extrap_ls(2, 1, 0), 4, "d + 2"))
CASES.append(Case("extrapolate_ls_simple-d2-inside-walls", _extrap_ls(2, 1, 1), 4, "d + 2"))


@case("vorticity_confinement", 4, "centred velocity (1) -> curl (1) -> gradient of its norm (1) -> force back on the faces (1)")
def _(c):
    vel = c.g("vel")
    c.call("mf_vorticity_confinement", *c.dims, vel, c.g("flags"), 0.4, None, c.zeros(3), c.zeros(3), c.zeros(1), c.zeros(3), None)
    return {"g_vel": vel}


def _shape_params(kind, sx, sy):
    q = {0: [3.2, 2.5, 5.3, sx - 4.1, sy - 2.7, 24.6], 1: [sx / 2, sy / 2, 14.3, 4.5, 1.0, 0.8, 1.7],
         2: [sx / 2, sy / 2, 15.2, 3.6, 0.0, 0.6, 0.8, 9.0]}[kind]
    return (ctypes.c_float * 12)(*(q + [0.0] * (12 - len(q))))


def _shape_levelset(kind):
    def fn(c):
        phi = c.zeros(1, fill=7)
        c.call("mf_shape_levelset", *c.dims, kind, _shape_params(kind, c.sx, c.sy), phi, None)
        return {"g_phi": phi}
    return fn


def _shape_apply(kind, gk):
    def fn(c):
        g = c.g("real") if gk == 0 else (c.g("flags") if gk == 3 else c.g("vec"))
        val = (ctypes.c_float * 3)(3.0, -1.5, 0.25)
        c.call("mf_shape_apply_to_grid", *c.dims, kind, _shape_params(kind, c.sx, c.sy), gk, g, val, c.g("flags") if gk != 3 else None, None)
        return {"g_grid": g}
    return fn


for _k, _nm in enumerate(("box", "sphere", "cylinder")):
    CASES.append(Case("shape_levelset-" + _nm, _shape_levelset(_k), 0, "cell-local, at the global cell centre", absz=True))
    for _gk, _gn in enumerate(("real", "vec3", "mac", "int")):
        CASES.append(Case("shape_apply_to_grid-%s-%s" % (_nm, _gn), _shape_apply(_k, _gk), 0, "cell-local, at the global cell centre", absz=True))


@case("grid_set_bound", 0, "cell-local; the z walls are the domain's", absz=True)
def _(c):
    g = c.g("real")
    c.call("mf_grid_set_bound", *c.dims, g, 0.75, 2, None)
    return {"g_grid": g}


@case("density_inflow", 0, "cell-local, noise at the global cell", absz=True)
def _(c):
    dens = c.g("real")
    c.call("mf_density_inflow", *c.dims, c.g("flags"), dens, c.g("phi"), c.tile(), c.noise_params(), 1.0, 1.5, None)
    return {"g_density": dens}


@case("apply_noise_vec3", 0, "cell-local, noise at the global cell centre", absz=True)
def _(c):
    t = c.g("vec")
    c.call("mf_apply_noise_vec3", *c.dims, c.g("flags"), t, c.tile(), c.noise_params(), 0.7, 1.3, None, 0, 0, 0, None, 0, 0, 0, None)
    return {"g_target": t}


@case("apply_noise_vec3-weight-same-size", 0, "cell-local (a weight grid of the target's size shares its window)", absz=True, same_src=True)
def _(c):
    t = c.g("vec")
    c.call("mf_apply_noise_vec3", *c.dims, c.g("flags"), t, c.tile(), c.noise_params(), 0.7, 1.3, c.g("real2"), *c.dims, None, 0, 0, 0, None)
    return {"g_target": t}


# (with a uv grid of the target's size the noise position is the uv value: nothing depends on absolute z, so no control)
@case("apply_noise_vec3-weight-uv-same-size", 0, "cell-local (weight and uv of the target's size share its window)", same_src=True)
def _(c):
    t = c.g("vec")
    c.call("mf_apply_noise_vec3", *c.dims, c.g("flags"), t, c.tile(), c.noise_params(), 0.7, 1.3, c.g("real2"), *c.dims, c.g("uv"), *c.dims, None)
    return {"g_target": t}


@case("apply_noise_vec3-coarse-weight", 0, "target 0; the source window holds the sampled planes +-1", absz=True)
def _(c):
    t = c.g("vec")
    c.call("mf_apply_noise_vec3", *c.dims, c.g("flags"), t, c.tile(), c.noise_params(), 0.7, 1.3, c.g("src_weight"), *c.sdims, None, 0, 0, 0, None)
    return {"g_target": t}


@case("apply_noise_vec3-coarse-weight-uv", 0, "target 0; the source window holds the sampled planes +-1", absz=True)
def _(c):
    t = c.g("vec")
    c.call("mf_apply_noise_vec3", *c.dims, c.g("flags"), t, c.tile(), c.noise_params(), 0.7, 1.3, c.g("src_weight"), *c.sdims,
           c.g("src_uv"), *c.sdims, None)
    return {"g_target": t}


def _interp(mac, ncomp, osp):
    def fn(c):
        f32 = np.float32         # calcGridSizeFactorMod with scale 1, offset 0 (plugins._size_factor): whole-domain sizes
        sf = [f32(f32(s) / f32(t)) for s, t in zip(SRC, (c.sx, c.sy, GSZ))]
        off = [f32(f * f32(0.5)) for f in sf]
        tgt = c.zeros(ncomp, fill=7)
        a = [float(v) for v in sf + off]
        if mac:
            c.call("mf_interpolate_mac_grid", *c.dims, tgt, *c.sdims, c.g("src_vec"), *a, osp, None)
        else:
            c.call("mf_interpolate_grid", *c.dims, tgt, *c.sdims, c.g("src_real" if ncomp == 1 else "src_vec"), ncomp, *a, osp, None)
        return {"g_target": tgt}
    return fn


for _os in (1, 2):
    _why = "target 0; the source window holds the sampled planes +-%d" % _os
    CASES.append(Case("interpolate_grid-real-space%d" % _os, _interp(False, 1, _os), 0, _why, absz=True))
    CASES.append(Case("interpolate_grid-vec3-space%d" % _os, _interp(False, 3, _os), 0, _why, absz=True))
    CASES.append(Case("interpolate_mac_grid-space%d" % _os, _interp(True, 3, _os), 0, _why, absz=True))


# ---- particle index and level set ------------------------------------------------------------------------------------------------
def _gpi(c):
    n = c.n()
    isys, index = c.impl.dev(np.zeros(n, np.int32)), c.zeros(1, np.int32)
    cnt = ctypes.c_int64(0)
    c.call("mf_grid_particle_index", *c.dims, n, n, c.p("pos"), c.p("pflag"), isys, index, c.zeros(1, np.int32),
           c.impl.dev(np.zeros(2 * n, np.int32)), c.impl.dev(np.zeros(2 * n, np.int32)), ctypes.byref(cnt), None)
    c.impl.sync()
    return isys, index, int(cnt.value)


@case("grid_particle_index", 0, "a particle belongs to its own cell", absz=True, check=check_gpi)
def _(c):
    isys, index, cnt = _gpi(c)
    return {"g_index": index, "x_isys": c.impl.host(isys)[:cnt].copy()}


def _union(rf):
    def fn(c):
        isys, index, cnt = _gpi(c)
        n = c.n()
        phi = c.zeros(1, fill=7)
        c.call("mf_union_particle_levelset", *c.dims, n, n, c.p("pos"), isys, cnt, index, phi, rf, c.p("ptype"), 4, None)
        return {"g_phi": phi}
    return fn


CASES.append(Case("union_particle_levelset-radius1.0", _union(1.0), 1, "r = int(radius) + 1 cells around each cell", absz=True))
CASES.append(Case("union_particle_levelset-radius2.5", _union(2.5), 2, "r = int(radius) + 1 cells around each cell", absz=True))


# ---- grid -> particles: compare the particles of the planes [lo + 1, hi - 1) --------------------------------------------------------
_G2P = "the trilinear stencil of a particle in plane k reads k - 1 .. k + 1"


@case("map_mac_to_parts", 1, _G2P, absz=True)
def _(c):
    n, pv = c.n(), c.p("pvel")
    c.call("mf_map_mac_to_parts", *c.dims, c.g("vel"), n, n, c.p("pos"), c.p("pflag"), pv, c.p("ptype"), 4, None)
    return {"p_pvel": pv}


@case("flip_velocity_update", 1, _G2P, absz=True)
def _(c):
    n, pv = c.n(), c.p("pvel")
    c.call("mf_flip_velocity_update", *c.dims, c.g("vel"), c.g("vec"), n, n, c.p("pos"), c.p("pflag"), pv, 0.97, c.p("ptype"), 4, None)
    return {"p_pvel": pv}


def _g2p(ncomp):
    def fn(c):
        n = c.n()
        t = c.p("preal" if ncomp == 1 else "pvel")
        c.call("mf_map_grid_to_parts", *c.dims, ncomp, c.g("real" if ncomp == 1 else "vec"), n, n, c.p("pos"), c.p("pflag"), t, None)
        return {"p_target": t}
    return fn


CASES.append(Case("map_grid_to_parts-real", _g2p(1), 1, _G2P, absz=True))
CASES.append(Case("map_grid_to_parts-vec3", _g2p(3), 1, _G2P, absz=True))


@case("apic_map_mac_to_parts", 1, _G2P, absz=True, pos="pos_apic")
def _(c):
    n, pv, cp = c.n(), c.p("pvel"), [c.p("cp0"), c.p("cp1"), c.p("cp2")]
    c.call("mf_apic_map_mac_to_parts", *c.dims, c.g("vel"), n, n, c.p("pos_apic"), c.p("pflag"), pv, cp[0], cp[1], cp[2], c.p("ptype"), 4, None)
    return {"p_pvel": pv, "p_cpx": cp[0], "p_cpy": cp[1], "p_cpz": cp[2]}


# ---- particles -> grid (deterministic mode): the windowed call gets the particles of [lo + 1, hi - 1), compare [lo + 2, hi - 2) -----
_P2G = ("a particle of plane k writes k - 1 .. k + 1; the call gets the particles of [lo + 1, hi - 1) because local_z clamps a stencil "
        "that leaves the window, so the planes [lo + 2, hi - 2) hold every contribution")


@case("map_parts_to_mac_accum", 2, _P2G, absz=True, feed=1)
def _(c):
    n, vel, w = c.n(), c.zeros(3, fill=7), c.zeros(3, fill=7)
    c.call("mf_map_parts_to_mac_accum", *c.dims, vel, w, n, n, c.p("pos"), c.p("pflag"), c.p("pvel"), c.p("ptype"), 4, 1, None)
    return {"g_vel": vel, "g_weight": w}


@case("apic_map_parts_to_mac", 2, _P2G, absz=True, feed=1, pos="pos_apic")
def _(c):
    n, vel, m = c.n(), c.zeros(3, fill=7), c.zeros(3, fill=7)
    c.call("mf_apic_map_parts_to_mac", *c.dims, vel, m, n, n, c.p("pos_apic"), c.p("pflag"), c.p("pvel"), c.p("cp0"), c.p("cp1"), c.p("cp2"),
           c.p("ptype"), 4, None)
    return {"g_vel": vel, "g_mass": m}


def _p2g(ncomp):
    def fn(c):
        n, t = c.n(), c.zeros(ncomp)
        c.call("mf_map_parts_to_grid", *c.dims, ncomp, t, c.zeros(1), n, n, c.p("pos"), c.p("pflag"), c.p("preal" if ncomp == 1 else "pvel"), 1, None)
        return {"g_target": t}
    return fn


CASES.append(Case("map_parts_to_grid-real", _p2g(1), 2, _P2G, absz=True, feed=1))
CASES.append(Case("map_parts_to_grid-vec3", _p2g(3), 2, _P2G, absz=True, feed=1))


# ---- other particle kernels -----------------------------------------------------------------------------------------------------
def _advect_parts(mode, delete, stop):
    def fn(c):
        n, pos, pf = c.n(), c.p("pos"), c.p("pflag")
        c.call("mf_advect_in_grid", *c.dims, c.g("flags"), c.g("vel"), n, n, pos, pf, DT, mode, delete, stop, 1, c.p("ptype"), 4,
               c.impl.dev(np.zeros(9 * n, np.float32)), None)
        return {"p_pos": pos, "p_pflag": pf}
    return fn


for _m, _mn in enumerate(("euler", "rk2", "rk4")):
    for _d in (0, 1):
        for _s in (0, 1):
            CASES.append(Case("advect_in_grid-%s-delete%d-stop%d" % (_mn, _d, _s), _advect_parts(_m, _d, _s), RP,
                              "ceil(max|v| dt) + 2 around the START cell: the path, the trilinear gather, the flag lookups of the obstacle bisection", absz=True))


def _mark_fluid(with_phi):
    def fn(c):
        n, fl = c.n(), c.g("flags_liquid")
        c.call("mf_mark_fluid_cells", *c.dims, fl, n, n, c.p("pos"), c.p("pflag"), c.p("ptype"), 4, c.g("phiObs") if with_phi else None,
               c.zeros(1, np.int32), None)
        return {"g_flags": fl}
    return fn


CASES.append(Case("mark_fluid_cells", _mark_fluid(False), 0, "a particle marks its own cell", absz=True))
CASES.append(Case("mark_fluid_cells-phiObs", _mark_fluid(True), 1, "the phiObs pass reads the six neighbours", absz=True))


@case("project_out_of_bnd", 0, "per particle; the z walls are the domain's", absz=True)
def _(c):
    n, pos = c.n(), c.p("pos")
    # bnd = 11.5: both z walls of the domain clamp particles that sit in the interior window [7, 20)
    c.call("mf_project_out_of_bnd", *c.dims, n, n, pos, c.p("pflag"), 11.5, 1 | 16 | 32, c.p("ptype"), 4, None)
    return {"p_pos": pos}


@case("push_out_of_obs", 1, "trilinear phiObs and its central-difference gradient", absz=True)
def _(c):
    n, pos = c.n(), c.p("pos")
    c.call("mf_push_out_of_obs", *c.dims, n, n, pos, c.p("pflag"), c.g("phiObs"), 0.05, 0.25, c.p("ptype"), 4, None)
    return {"p_pos": pos}


@case("set_part_type", 0, "the flag of the particle's own cell", absz=True)
def _(c):
    n, pt = c.n(), c.p("ptype")
    c.call("mf_set_part_type", *c.dims, c.g("flags"), n, n, c.p("pos"), pt, 4, 1, util.OBS | util.EMPTY, None)
    return {"p_ptype": pt}


@case("reset_outflow", 0, "the flag of the particle's own cell", absz=True, pos="pos_out")
def _(c):
    n = c.n("pos_out")
    fl, phi, real, pf = c.g("flags_out"), c.g("phi"), c.g("real"), c.p("pflag_out")
    c.call("mf_reset_outflow", *c.dims, fl, phi, real, n, n, c.p("pos_out"), pf, None)
    return {"g_flags": fl, "g_phi": phi, "g_real": real, "p_pflag": pf}


@case("plugins.resetOutflow", 0, "the flag of the particle's own cell", absz=True, pos="pos_out")
def _(c):
    from mantaflow_amd import core, plugins
    import cases
    with c.package() as s:
        fl = cases.soa_to_grid(core.FlagGrid(s), c.g("flags_out").cpu().numpy())
        phi, real = cases.soa_to_grid(core.Grid(s), c.g("phi").cpu().numpy()), cases.soa_to_grid(core.Grid(s), c.g("real").cpu().numpy())
        pp = cases._mk_parts(s, c.A["pos_out"].copy(), c.A["pflag_out"].copy())
        plugins.resetOutflow(flags=fl, phi=phi, parts=pp, real=real)
        s.sync()
        return {"g_flags": fl.data.cpu().numpy().copy(), "g_phi": phi.data.cpu().numpy().copy(), "g_real": real.data.cpu().numpy().copy(),
                "p_pflag": pp.flag[:pp.np].cpu().numpy().copy()}


BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# (case, plane shape): every case on 15 x 11; on 16 x 12 the ones whose HIP kernels branch on the 16-byte alignment of a plane or
# vectorise along x (the extrapolations, the semi-Lagrange z-columns, the fused MacCormack kernels, the deterministic scatters)
ALIGNED = ("semi_lagrange_", "maccormack_correct_clamp", "extrapolate_", "map_parts_to_mac_accum", "mark_fluid_cells", "vorticity")
PARAMS = [(c.name, "15x11") for c in CASES] + [(c.name, "16x12") for c in CASES if c.name.startswith(ALIGNED)]


# ---------------------------------------------------------------------------------------------------------------------------
# the checks the two test files run
# ---------------------------------------------------------------------------------------------------------------------------
def check_oracle(oracle, name, shape, win):
    """oracle windowed == oracle undivided on the trimmed range; the cut is live; the window matters"""
    case = BY_NAME[name]
    what = "%s %s %s" % (name, shape, win)
    und, got = run_cached(oracle, case, shape), run_cached(oracle, case, shape, win)
    check_window(case, shape, win, und, got, what)
    lo, hi = WINDOWS[win]
    if case.reach > 0 and ((lo > 0 and "lo" in case.sides) or (hi < GSZ and "hi" in case.sides)):
        assert differs(case, shape, win, und, got, False), "%s: nothing differs in the %d planes trimmed away: the cut is not live" % (what, case.reach)
    if case.absz and lo > 0:
        # with lo == 0 the offset is the identity and only gsz tells a window from none, which most of these kernels never read
        ctl = run(oracle, case, shape, win, window_set=False)
        if case.check is None:
            assert differs(case, shape, win, und, ctl, True), "%s: the same call without a window gives the same result: the case does not depend on z" % what
        else:
            try:
                case.check(case, shape, win, und, ctl, what)
            except AssertionError:
                pass
            else:
                raise AssertionError("%s: the same call without a window passes" % what)


def check_hip(hip, oracle, name, shape, win):
    """HIP windowed == oracle undivided on the trimmed range, HIP windowed == oracle windowed everywhere"""
    case = BY_NAME[name]
    what = "%s %s %s" % (name, shape, win)
    got = run(hip, case, shape, win)
    check_window(case, shape, win, run_cached(oracle, case, shape), got, what + " [hip]")
    check_whole(got, run_cached(oracle, case, shape, win), what + " [hip vs oracle]")
