"""Every kernel family on a caller's non-blocking stream: the helpers and the case table of tests/test_gpu_streams.py, and what
tests/test_stream_cases.py checks without a GPU.

PyTorch side streams are created non-blocking: the null stream does not wait for them and they do not wait for it.  Inside
`side_stream()` the package hands the library the side stream (core._stream reads the current stream), and `StreamImpl` does the same for
the raw-ABI runners, which pass None for `stream`.  So any work the library queues on the null stream instead (a hipMemset of a fresh
buffer, say) is no longer ordered with its kernels by accident.  `busy()` makes that visible every time rather than sometimes: a chain of
element-wise kernels on the default stream that outlasts the case, behind which a null-stream fill would land on top of the case's output.

Each entry of CASES is (id, files, run, check, solve, device_syncs):
  files         the csrc/*.hip files whose kernels the case launches (tests/test_stream_cases.py asks that every file with kernels is named)
  run()         drives the HIP library on the current stream; reuses the family's existing runner at the smallest size its GPU test uses
  check(got)    compares with the reference the family's existing test uses -- the plain-C oracle on the same inputs (computed once and
                cached here), the numpy model or the golden file -- at that test's bar.  Nothing expected comes from a run of the HIP library.
                Where the family's test body interleaves device calls with its comparisons, run() is that body on its smallest case
                (a `hip_backend` argument is given as None) and there is nothing left for check() to do.
  solve         a Flag where the case runs MIC sweeps or a PCG: never run beside the busy chain ("Concurrency contract")
  device_syncs  a Flag where the case calls an entry that holds a hipDeviceSynchronize: "the chain is still running" cannot hold
A Flag names the file and line that decide it and a word that line must contain.

The busy chain.  Measured on an MI355X with a pair of events around 200 operations: one in-place multiply by 1.0 of the 2^28-float tensor
takes 0.36 ms (BUSY_OP_SECONDS; 0.3603 to 0.3610 ms in three runs, 0.9 ms of host time to queue the 200).  The slowest table case on the
default stream with the parent commit's library, second run in the process, takes 0.263 s of wall time (SLOWEST_CASE_SECONDS: mg2d-stages,
whose body computes the numpy model of the hierarchy between its device calls; the next slowest are runtime-reductions-and-elementwise
with 0.027 s and meshops-smooth with 0.020 s, most cases take 1 to 5 ms).  SPAN is three times that, rounded up: 0.8 s, 2223 operations.
"""
import collections
import contextlib
import ctypes
import functools
import importlib
import math
import os

import numpy as np
import torch

import cases
import util
from util import assert_bitexact, rel_err

Flag = collections.namedtuple("Flag", "file line call")
Case = collections.namedtuple("Case", "id files run check solve device_syncs")

BUSY_ELEMS = 1 << 28
BUSY_OP_SECONDS = 0.36e-3
SLOWEST_CASE_SECONDS = 0.263
SPAN = 0.8
assert SPAN >= 3 * SLOWEST_CASE_SECONDS

TOL = 1e-5      # test_gpu_parity.TOL


# ---- streams ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def side_stream(stream=None):
    """one new (non-blocking) stream -- or the one given -- as the current one; on the way out it is synchronised and the previous stream
    is current again"""
    S = stream if stream is not None else torch.cuda.Stream()
    with torch.cuda.stream(S):
        try:
            yield S
        finally:
            S.synchronize()


_beside = []


def stream_beside_default():
    """a side stream whose work does not queue up behind the default stream's.  The runtime spreads its streams over a few hardware
    queues (GPU_MAX_HW_QUEUES), so some streams of torch's pool share the null stream's queue and run in order with it, non-blocking or
    not: correct, but nothing can run *beside* a busy default stream there.  Found by condition, once per process: a kernel on the
    candidate completes while a short chain on the default stream is still running."""
    if not _beside:
        for _ in range(12):
            st = torch.cuda.Stream()
            ev = busy(torch.cuda.default_stream(), 0, ops=100)
            with torch.cuda.stream(st):
                torch.zeros(16, device="cuda")
            st.synchronize()
            beside = not ev.query()
            ev.synchronize()
            if beside:
                _beside.append(st)
                break
        else:
            raise AssertionError("no stream of twelve ran beside the default stream")
    return _beside[0]


_busy_tensor = []


def busy_ops(span):
    return int(math.ceil(span / BUSY_OP_SECONDS))


def busy(stream, span, ops=None):
    """queue about `span` seconds of in-place multiplies by 1.0 of one large tensor on `stream`; -> an event recorded after the last.
    A finite chain of plain element-wise kernels: nothing polls, nothing persists, no host callback."""
    if not _busy_tensor:
        _busy_tensor.append(torch.ones(BUSY_ELEMS, dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()                     # once: the tensor is filled before any stream multiplies it
    x = _busy_tensor[0]
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        for _ in range(busy_ops(span) if ops is None else ops):
            x.mul_(1.0)
        ev.record(stream)
    return ev


def current_stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _arg_names():
    from mantaflow_amd import _lib
    names = {k: v[2] for k, v in _lib.parse_header().items()}
    for ext in _lib.all_extensions():
        names.update({k: v[2] for k, v in _lib.parse_header(ext.header).items()})
    return names


class StreamImpl(util.Impl):
    """util.Impl("hip") for the existing raw-ABI runners, which pass None for `stream` and synchronise the device: here a None in the
    place of an entry's trailing `stream` argument becomes the current torch stream, and sync() waits for that stream alone"""

    def __init__(self):
        util.Impl.__init__(self, "hip")

    def call(self, name, *args):
        names = _arg_names().get(name, ())
        if names and names[-1] in ("stream", "s") and len(args) == len(names) and args[-1] is None:
            args = args[:-1] + (current_stream_ptr(),)
        return util.Impl.call(self, name, *args)

    def sync(self):
        torch.cuda.current_stream().synchronize()


@functools.lru_cache(maxsize=None)
def simpl():
    return StreamImpl()


@contextlib.contextmanager
def poisoned_pools():
    """every solver made inside starts with a pool of NaN / 0x7f7f7f7f tensors (cases.poison_pool), so scratch that a kernel reads before
    its producer wrote it is no plausible old value"""
    from mantaflow_amd import core
    init = core.FluidSolver.__init__

    def poisoned(self, *a, **kw):
        init(self, *a, **kw)
        if self.device != "cpu":
            cases.poison_pool(self)

    core.FluidSolver.__init__ = poisoned
    try:
        yield
    finally:
        core.FluidSolver.__init__ = init


# ---- references --------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(key, thunk):
    """thunk() with the package routed through the plain-C oracle; once per key"""
    if key not in _ORACLE:
        from mantaflow_amd import _lib
        _lib.use_library(util.build_oracle(), "cpu")
        try:
            _ORACLE[key] = thunk()
        finally:
            _lib.reset()
    return _ORACLE[key]


@functools.lru_cache(maxsize=None)
def _oracle_impl():
    return util.Impl("oracle")


def _same(got, want, what):
    if isinstance(want, dict):
        for k in want:
            assert_bitexact(got[k], want[k], "%s: %s" % (what, k))
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want), what
        for q, (g, w) in enumerate(zip(got, want)):
            assert_bitexact(g, w, "%s[%d]" % (what, q))
    else:
        assert_bitexact(got, want, what)


def _close(a, b, what, tol=TOL):
    e = rel_err(a, b)
    assert e <= tol, "%s: relative error %g > %g" % (what, e, tol)


def _T(name):
    return importlib.import_module(name)


def _golden(path):
    return np.load(path)


CASES = []


def _case(id, files, run, check=None, solve=None, device_syncs=None):
    CASES.append(Case(id, tuple(files), run, check or (lambda got: None), solve, device_syncs))


def _pkg_vs_oracle(id, files, thunk, compare=_same, **flags):
    """thunk() through the package on whichever backend is active: HIP on the current stream against the oracle"""
    _case(id, files, thunk, lambda got: compare(got, _oracle(id, thunk), id), **flags)


PCG = Flag("mantaflow_amd/csrc/pressure.hip", 1572, "mf_cg_solve")
PCG_PKG = Flag("mantaflow_amd/plugins.py", 485, "mf_solve_pressure_fused")
PCG_DIFFUSION = Flag("mantaflow_amd/plugins.py", 329, "mf_cg_solve")
PCG_MG = Flag("mantaflow_amd/csrc/mg_driver.h", 433, "cg_solve_external")
PCG_VIC = Flag("mantaflow_amd/vortexsheet.py", 409, "mf_cg_solve")
SWEEP = Flag("mantaflow_amd/csrc/mic.hip", 1715, "mf_mic_apply")
MG_CREATE = Flag("mantaflow_amd/csrc/mg_driver.h", 368, "hipDeviceSynchronize")
MG_DESTROY = Flag("mantaflow_amd/csrc/mg_driver.h", 393, "hipDeviceSynchronize")


# ---- the base families: the runners of tests/cases.py against the oracle ----------------------------------------------------------------
def _advect(kind):
    dims = (14, 12, 10)
    flags, vel = cases.advect_inputs(dims, 9, vmax=2.5, outflow=(kind == 2))
    field = util.rand_real(dims[::-1], 10) if kind == 0 else util.rand_vel(*dims, 10)
    return lambda: cases.run_advect_pkg(dims, 0.9, flags, vel, field, kind, order=2, clampMode=2, orderTrace=1, strength=0.8)


_pkg_vs_oracle("advect-real-maccormack", ["advect"], lambda: _advect(0)())
_pkg_vs_oracle("advect-mac-maccormack-outflow", ["advect"], lambda: _advect(2)())


def _flip():
    dims = (12, 10, 9)
    flags = util.make_flags(*dims, 14, empty_top=True)
    vel, velOld = util.rand_vel(*dims, 15), util.rand_vel(*dims, 16)
    pos, pflag, pvel = util.make_particles(flags, 3, 17)
    return cases.run_flip_pkg(dims, flags, vel, velOld, pos, pflag, pvel, None, 0, deterministic=True)


_pkg_vs_oracle("flip-transfers", ["flip", "p2g_ordered"], _flip)


def _apic():
    dims = (12, 10, 9)
    flags, vel, pos, pflag, pvel, cp = cases.apic_inputs(dims, 61, 3, include_border=False)
    return cases.run_apic_pkg(dims, flags, vel, pos, pflag, pvel, cp, None, 0)


_pkg_vs_oracle("flip-apic", ["flip", "p2g_ordered"], _apic)


def _advect_parts():
    dims = (12, 10, 9)
    flags = util.make_flags(*dims, 19, empty_top=True)
    vel = util.smooth_vel(*dims, 20, 2.0)
    pos, pflag, _ = util.make_particles(flags, 2, 21)
    return cases.run_advect_parts_pkg(dims, 0.8, flags, vel, pos, pflag, 2, True, True)


_pkg_vs_oracle("flip-advect-in-grid", ["flip"], _advect_parts)


def _p2g_ordered_run():
    OC = _T("p2g_ordered_cases")
    out = {}
    for entry in ("mac", "grid3"):
        out.update(OC.run_entry(simpl(), OC.get("runs64-dyadic"), entry))
    out.update(OC.run_entry(simpl(), OC.get("apic-shapes-17x11x9-dyadic"), "apic"))
    return out


def _p2g_ordered_check(got):
    OC = _T("p2g_ordered_cases")
    want = dict(OC.oracle_outputs("runs64-dyadic"))
    want.update(OC.oracle_outputs("apic-shapes-17x11x9-dyadic", None, True))
    for k, v in got.items():
        inp = OC.get("apic-shapes-17x11x9-dyadic" if k.startswith("apic") else "runs64-dyadic")
        OC.assert_same(inp, v, want[k], "%s vs the serial scatter" % k)


_case("p2g-ordered-entries", ["p2g_ordered"], _p2g_ordered_run, _p2g_ordered_check)

_pkg_vs_oracle("surface-pieces", ["surface", "scan"], lambda: cases.run_surface_pkg((14, 12, 10), cases.surface_inputs((14, 12, 10), 51)))
_pkg_vs_oracle("surface-reset-outflow", ["surface"], lambda: cases.run_outflow_pkg((14, 12, 10), *cases.outflow_inputs((14, 12, 10), 71)))


def _interp():
    sd, td, scale, offset, size = cases.INTERP_CASES[0]
    fields = {"real": util.rand_real((sd[2], sd[1], sd[0]), 71), "vec": util.rand_vel(*sd, 72)}
    return cases.run_interp_pkg(sd, td, scale, offset, size, fields, 1)


_pkg_vs_oracle("surface-interpolate-grid", ["surface"], _interp)


def _glue():
    dims = (12, 10, 9)
    flags = util.make_flags(*dims, 26, empty_top=True)
    flags[flags.shape[0] // 2, 3, 3] |= util.STICK
    return cases.run_glue_pkg(dims, 0.7, flags, util.rand_vel(*dims, 27), util.rand_real(dims[::-1], 28))


_pkg_vs_oracle("glue", ["glue"], _glue)
_pkg_vs_oracle("glue-flip", ["glue"], lambda: cases.run_flipglue_pkg((14, 12, 10), *cases.flipglue_inputs((14, 12, 10), 31), None))


def _runtime_check(got):
    cases.check_reductions(got, cases.run_reductions_impl(_oracle_impl(), *cases.reduction_inputs()))


_case("runtime-reductions-and-elementwise", ["runtime"], lambda: cases.run_reductions_impl(simpl(), *cases.reduction_inputs()), _runtime_check)


def _turb():
    dims, small = (20, 14, 12), (10, 7, 6)
    return cases.run_turb_pkg(dims, *cases.turb_inputs(dims, small, 91), small)


_pkg_vs_oracle("noise-turbulence-pieces", ["noise", "turbulence"], _turb)


# ---- pressure and MIC: raw entries with the stream argument, and solvePressure ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _system(dims):
    flags, A, src = cases.system_inputs(dims, 5)
    return flags, A, src, cases.cg_rhs(dims, flags, 5)


def _cg(impl, dims, pc):
    flags, A, _, rhs = _system(dims)
    return cases.run_cg_impl(impl, dims, flags, A, rhs, pc, 1e-3, 60 if pc else 80, 0)


def _cg_check(dims, pc):
    def check(got):
        (x, st), (xo, sto) = got, _cg(_oracle_impl(), dims, pc)
        assert st[0] == sto[0], (st, sto)
        _close(x, xo, "cg solution")
        _close(st[1:], sto[1:], "resNorm/sigma", 1e-4)
    return check


def _cg_case(dims, pc):
    _case("pressure-cg-pc%d-%dx%dx%d" % ((pc,) + dims), ["pressure", "mic"] if pc else ["pressure"], lambda: _cg(simpl(), dims, pc),
          _cg_check(dims, pc), solve=PCG)


for _dims in ((16, 16, 16), (12, 10, 9)):       # rows of a multiple of 8 cells, and the padded internal copy
    for _pc in (2, 0):
        _cg_case(_dims, _pc)


def _solve_pressure(liquid):
    dims = (12, 10, 9)
    flags, vel, phi = cases.pressure_inputs(dims, 6, liquid)
    return cases.run_solve_pressure_pkg(dims, flags, vel, phi)


def _solve_pressure_same(got, want, what):
    assert got["stats"]["iterations"] == want["stats"]["iterations"], (got["stats"], want["stats"])
    assert_bitexact(got["rhs"], want["rhs"], "rhs")
    _close(got["pressure"], want["pressure"], "pressure")
    _close(got["vel"], want["vel"], "vel")


_pkg_vs_oracle("pressure-solve-plain", ["pressure", "mic"], lambda: _solve_pressure(False), _solve_pressure_same, solve=PCG)
_pkg_vs_oracle("pressure-solve-liquid", ["pressure", "mic"], lambda: _solve_pressure(True), _solve_pressure_same, solve=PCG)


def _solve_pressure_fused():
    dims = (32, 24, 16)
    flags, vel, _ = cases.pressure_inputs(dims, 21, False)
    return cases.run_solve_pressure_pkg(dims, flags, vel, None)


_pkg_vs_oracle("pressure-solve-fused-setup", ["pressure", "mic"], _solve_pressure_fused, _solve_pressure_same, solve=PCG_PKG)


def _diffusion():
    dims = (14, 12, 10)
    flags = util.make_flags(*dims, 81, obstacles=True)
    return cases.run_diffusion_pkg(dims, flags, util.rand_real(dims[::-1], 82), util.rand_vel(*dims, 83))


def _diffusion_same(a, b, what):
    assert (a["iters"] == b["iters"]).all(), (a["iters"], b["iters"])
    _close(a["real"], b["real"], "diffused Real grid")
    _close(a["mac"], b["mac"], "diffused MAC grid")


_pkg_vs_oracle("pressure-cg-diffusion", ["pressure"], _diffusion, _diffusion_same, solve=PCG_DIFFUSION)

MIC_DIMS = [(16, 16, 16), (20, 13, 11)]      # rows of a multiple of 8 cells, and not


def _mic(impl, dims, mode):
    flags, A, src, _ = _system(dims)
    if impl.which == "hip":
        assert impl.lib.cdll.mf_set_mic_mode(mode.encode()) == 0
    try:
        return cases.run_mic_impl(impl, dims, flags, A, src)
    finally:
        if impl.which == "hip":
            assert impl.lib.cdll.mf_set_mic_mode(None) == 0


def _mic_case(dims, mode):
    def check(got):
        want = _mic(_oracle_impl(), dims, mode)
        assert_bitexact(got[0], want[0], "Aprecond " + mode)
        assert_bitexact(got[1], want[1], "mic apply " + mode)
    _case("mic-%s-%dx%dx%d" % ((mode,) + dims), ["mic"], lambda: _mic(simpl(), dims, mode), check, solve=SWEEP)


for _dims in MIC_DIMS:
    for _mode in ("rows", "levels"):
        _mic_case(_dims, _mode)


# ---- multigrid ----------------------------------------------------------------------------------------------------------------------------
def _mg_stages():
    """create -> set_a -> info / read_level -> vcycle -> destroy through the C ABI: the body of test_stages_equal_reference"""
    mg_cases = _T("mg_cases")
    return _T("test_gpu_multigrid").test_stages_equal_reference(simpl(), _golden(mg_cases.GOLDEN), "obs")


_case("multigrid-stages", ["multigrid"], _mg_stages, device_syncs=MG_CREATE)


def _mg_solve():
    mg_cases = _T("mg_cases")
    dims = (12, 10, 9)
    flags, vel, phi, kw = mg_cases.inputs("obs", dims)
    return mg_cases.run_pkg(dims, flags, vel, phi, preconditioner=mg_cases.PcMGDynamic, **kw)


def _mg_solve_check(got):
    """create -> set_a -> cg_solve (V-cycles inside) through solvePressure: the recorded reference's iterations and digests"""
    mg_cases = _T("mg_cases")
    g, name = _golden(mg_cases.GOLDEN), mg_cases.case_name("obs", (12, 10, 9))
    assert got["iterations"] == int(g["iters__" + name]) < 100
    assert mg_cases.sha256(got["pressure"]) == bytes(g["sha_p__" + name]).hex(), "pressure differs from the reference's"
    assert mg_cases.sha256(got["vel"]) == bytes(g["sha_v__" + name]).hex(), "velocity differs from the reference's"


_case("multigrid-solve", ["multigrid", "pressure"], _mg_solve, _mg_solve_check, solve=PCG_MG, device_syncs=MG_CREATE)


def _mg2d_stages():
    C = _T("mg2d_cases")
    return _T("test_gpu_mg2d").test_levels_equal_reference_and_model(simpl(), _golden(C.GOLDEN), "obs_30x30x1__lap")


_case("mg2d-stages", ["mg2d"], _mg2d_stages, device_syncs=MG_CREATE)
_case("mgslab-cut-form", ["mgslab", "multigrid"], lambda: _T("test_gpu_mgslab").check_cut_form(simpl(), (24, 20, 18), "lap", (9,)),
      device_syncs=MG_DESTROY)


# ---- the extension families: each against the reference its own GPU test uses ------------------------------------------------------------
def _reinit_run():
    import manta as m
    T, M = _T("test_gpu_reinit"), _T("reinit_model")
    assert "MF_REINIT_SERIAL" not in os.environ
    name = list(M.CASES)[0]
    c = M.case(name)
    dims = c["dims"]
    s = m.Solver(name="t", gridSize=m.vec3(*dims), dim=2 if dims[2] == 1 else 3)
    g = {"phi": s.create(m.LevelsetGrid), "flags": s.create(m.FlagGrid), "vel": s.create(m.MACGrid)}
    T._load(g["flags"].data, c["flags"])
    T._poison(s, c["velocity"] is not None)
    return T._call(m, g, c, c["phi"], c["velocity"])


def _reinit_check(got):
    T, M = _T("test_gpu_reinit"), _T("reinit_model")
    name = list(M.CASES)[0]
    phi, vel, fm, key, st = got
    assert T._same(name, "phi", phi) and (vel is None or T._same(name, "vel", vel)), name
    assert T._same(name, "fm", fm.astype(np.int8)) and T._same(name, "key", key), name
    want = {k: tuple(int(x) for x in row) for k, row in zip(("windows", "subrounds", "pops", "serial"), T.G[name + "/stats"])}
    assert st == want, (st, want)


_case("reinit-marching", ["reinit"], _reinit_run, _reinit_check)


def _resample_run():
    import manta as m
    T, M = _T("test_gpu_nbflip"), _T("nbflip_model")
    name, allow = M.ADJUST_RUNS[0]
    I, calls = M.adjust_case(name, allow)
    cname = list(M.COMBINE_CASES)[0]
    J = M.combine_inputs(cname)
    s = T._solver(m, M.COMBINE_CASES[cname][0])
    vel, w, comb = T._grid(s, m.MACGrid, J["vel"]), T._grid(s, m.MACGrid, J["weight"]), T._grid(s, m.MACGrid, J["comb"])
    phi = T._grid(s, m.LevelsetGrid, J["phi"]) if J["phi"] is not None else None
    m.combineGridVel(vel=vel, weight=w, combineVel=comb, phi=phi, narrowBand=J["narrowBand"], thresh=J["thresh"])
    return T._run_device(m, I, calls, M.ADJUST_CASES[name][0]), vel.to_numpy(), comb.to_numpy()


def _resample_check(got):
    T, M = _T("test_gpu_nbflip"), _T("nbflip_model")
    name, allow = M.ADJUST_RUNS[0]
    cname = list(M.COMBINE_CASES)[0]
    for ci, st in enumerate(got[0]):
        for k in ("pos", "flag", "ch0", "ch1", "ch2", "ch3", "book"):
            T._same(st[k], T.GOLDEN["adjust/%s/%d/%d/%s" % (name, int(allow), ci, k)], "%s call %d %s" % (name, ci, k))
    T._same(got[1], T.GOLDEN["combine/%s/vel" % cname], cname + " vel")
    T._same(got[2], T.GOLDEN["combine/%s/comb" % cname], cname + " combineVel")


_case("resample-adjust-number-and-combine", ["resample", "scan"], _resample_run, _resample_check)


def _obstacles_names():
    M = _T("obstacle_model")
    first = {}
    for name in M.CASES:
        first.setdefault(M.CASES[name][0], name)      # the first fixture case of each of the five plugins
    return list(first.values())


def _obstacles_run():
    T, M = _T("test_gpu_obstacles"), _T("obstacle_model")
    return {name: T.run_pkg(M.CASES[name][0], M.CASES[name][1], M.case_inputs(name), M.CASES[name][3]) for name in _obstacles_names()}


def _obstacles_check(got):
    T, M = _T("test_gpu_obstacles"), _T("obstacle_model")
    for name, v in got.items():
        assert_bitexact(v[0] if M.CASES[name][0] == "addNoise" else v, T.GOLDEN[name], name)


_case("obstacles-fixture-cases", ["obstacles", "noise"], _obstacles_run, _obstacles_check)


def _idp_names():
    M = _T("idp_model")
    first = {}
    for name in M.CASES:
        first.setdefault(M.CASES[name][0], name)      # one fixture case per plugin (mark, mass, delta, pos)
    return list(first.values())


def _idp_run():
    import manta as m
    T, M = _T("test_gpu_idp"), _T("idp_model")
    return {name: T.run_case(m, M.CASES[name][0], M.CASES[name][1], M.case_inputs(name), M.CASES[name][3])[0] for name in _idp_names()}


def _idp_check(got):
    T = _T("test_gpu_idp")
    for name, out in got.items():
        for k, v in out.items():
            assert_bitexact(v, T.GOLDEN[name + "/" + k], name + "/" + k)


_case("idp-fixture-cases", ["idp"], _idp_run, _idp_check)


def _partls_name():
    M = _T("partls_model")
    return next(n for n in M.CASES if not M.CASES[n]["improved"])      # averagedParticleLevelset: compared bit for bit


def _partls_run():
    import manta as m
    T, M = _T("test_gpu_partls"), _T("partls_model")
    name = _partls_name()
    return T.Scene(m, M.CASES[name]["dims"], M.case_inputs(name)).run(False, **M.case_kwargs(name))


_case("partls-averaged", ["partls", "surface"], _partls_run, lambda got: assert_bitexact(got, _T("test_gpu_partls").GOLDEN[_partls_name() + "/phi"], "phi"))
_case("partls-improved", ["partls", "surface"], lambda: _T("test_gpu_partls").check_fixture_case(
    __import__("manta"), next(n for n in _T("partls_model").CASES if _T("partls_model").CASES[n]["improved"])) is None)


def _guiding_inputs():
    T, M = _T("test_gpu_guiding"), _T("guiding_model")
    dims, radius = T.BLUR_SHAPES[0]
    sx, sy, sz = dims
    a = np.random.RandomState(radius + sx * sy * sz).uniform(-2, 2, (sz, sy, sx, 3)).astype(np.float32)
    return dims, radius, a, T.flag_grids(dims)["random"], M.weights(radius)


def _guiding_run():
    """mf_guiding_blur (the three separable passes, twice) with the stream argument"""
    from mantaflow_amd import _lib
    T = _T("test_gpu_guiding")
    dims, radius, a, flags, w = _guiding_inputs()
    sx, sy, sz = dims
    n = sx * sy * sz
    fl, grid, w_dev = T.dev(flags), T.dev(T.soa(a)), T.dev(w)
    s1, s2 = (torch.full((3 * n,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
    _lib.get().call("mf_guiding_blur", sx, sy, sz, T.P(fl), T.P(grid), T.P(s1), T.P(s2), T.P(w_dev), radius, 2, current_stream_ptr())
    return T.aos(grid, (sz, sy, sx))


def _guiding_check(got):
    M = _T("guiding_model")
    dims, radius, a, flags, w = _guiding_inputs()
    assert_bitexact(got, M.blur(a, flags, w, dims[2] > 1, 2), "blur")


_case("guiding-blur", ["guiding"], _guiding_run, _guiding_check)


def _secparts_name():
    return sorted(_T("secparts_model").POT_CASES)[0]


def _secparts_run():
    import manta as m
    return _T("test_gpu_secparts").run_potentials(m, _T("secparts_model").pot_inputs(_secparts_name()))


def _secparts_check(got):
    T = _T("test_gpu_secparts")
    for k, v in got.items():
        T.bits_equal(_secparts_name() + "/" + k, v, T.GOLDEN[_secparts_name() + "/" + k])


_case("secparts-potentials", ["secparts"], _secparts_run, _secparts_check)

_case("turbulence-model-sources-and-bcs", ["turbulence_model"],
      lambda: _T("test_gpu_turbulence").test_sources_and_bcs(None, _T("turbulence_model").SOURCES_CASES[0]))
_case("turbulence-model-gradient-diffusion", ["turbulence_model"],
      lambda: _T("test_gpu_turbulence").test_gradient_diffusion_twice(None, _T("turbulence_model").GRADDIFF_CASES[0], True))
_case("fields-fire", ["fields"], lambda: _T("test_gpu_fields").test_process_burn_and_update_flame(None, "g7/all"))


def _mesh_name():
    M = _T("mesh_model")
    return min((n for n in M.CASES if M.model_mesh(n)[0]["tris"].shape[0] > 0), key=lambda n: M.case_phi(n).size)


_case("mesh-create", ["mesh", "scan"], lambda: _T("test_gpu_mesh").test_create_mesh_cases(None, _mesh_name()))
_case("mesh-advect-in-grid", ["mesh"], lambda: _T("test_gpu_mesh").test_advect_in_grid(None, 65))
_case("meshops-connectivity", ["meshops", "scan"],
      lambda: _T("test_gpu_meshops").test_connectivity_cases(None, "sphere17"))
_case("meshops-smooth", ["meshops", "scan"], lambda: _T("test_gpu_meshops").test_smooth_cases(None, "sphere17"))
_case("meshsdf-level-set", ["meshsdf", "scan"], lambda: _T("test_gpu_meshsdf")._run_case(__import__("manta"), "rand65") and None)


def _grid4d_cases():
    M = _T("grid4d_model")
    all_cases = list(M.op_cases())
    shape = all_cases[0][1]
    return [c for c in all_cases if c[1] == shape and c[3] == "real"]      # every operator, reduction and boundary rule on one shape


def _grid4d_run():
    import manta as m
    T = _T("test_gpu_grid4d")
    todo = _grid4d_cases()
    s = T._solver(m, todo[0][2])
    return {key: T._run_op(m, s, dims, kind, op, arg) for key, name, dims, kind, op, arg in todo}


def _grid4d_check(got):
    T, M = _T("test_gpu_grid4d"), _T("grid4d_model")
    for key, v in got.items():
        msg = M.same_as_fixture(T.GOLDEN, key, v)
        assert msg is None, msg


_case("grid4d-operators-and-reductions", ["grid4d"], _grid4d_run, _grid4d_check)
_case("gridops-permute", ["gridops"], lambda: _T("test_gpu_gridops").test_permute_fixture_cases(None, next(c for c in _T("gridops_model").permute_cases() if c[0] == "perm/in/5x5x5/120/vec")))


def _movingobs_run():
    import manta as m
    T, M = _T("test_gpu_movingobs"), _T("movingobs_model")
    g = T.GRIDS[0]
    s = T.solver(m, g)
    f, v, o = M.wall2_inputs(g)
    flags, vel, obvel = T.grid_from(s, m.FlagGrid, f), T.grid_from(s, m.MACGrid, v), T.grid_from(s, m.MACGrid, o)
    m.set_wall_bcs2(flags, vel, obvel=obvel)
    return vel.to_numpy()


_case("movingobs-wall-bcs2", ["movingobs"], _movingobs_run,
      lambda got: _T("test_gpu_movingobs").same("vel", got, _T("test_gpu_movingobs").GOLDEN["wall2/" + _T("test_gpu_movingobs").GRIDS[0]]))
_case("movingobs-extrapolate", ["movingobs"], lambda: _T("test_gpu_movingobs").test_extrapolate_with_phi_obs(None, _T("test_gpu_movingobs").GRIDS[0]))
_case("mlflip-features", ["mlflip"], lambda: _T("test_gpu_mlflip").test_features_fixture_cases(None, "f3d_w1"))
_case("mlflip-regions", ["mlflip"], lambda: _T("test_gpu_mlflip").test_regions_fixture_cases(None, "r7x5x4"))
_case("datagen-blur", ["datagen"], lambda: _T("test_gpu_datagen").test_blur(None, *next(c for c in _T("datagen_model").blur_cases() if c[0] == "row67")))
_case("datagen-center-of-mass", ["datagen"], lambda: _T("test_gpu_datagen").test_center_of_mass(None, _T("datagen_model").COM_CASES[0]))


def _vortex_velocity():
    T = _T("test_gpu_vortex")
    name = "self65"
    T._checked.pop(name, None)          # the test caches its verdict per process: this run has to reach the device
    T._velocity_check(name)


_case("vortex-velocity", ["vortex"], _vortex_velocity)
_case("vortex-density-from-levelset", ["vortex"],
      lambda: _T("test_gpu_vortex").test_density_from_levelset(None, list(_T("vortex_model").DENSITY_CASES)[0]))
_case("vsheet-stages", ["vsheet"], lambda: _T("test_gpu_vsheet").test_recorded_stage_cases(None, "sphere17"))
_case("vsheet-vic-solve", ["vsheet", "pressure"],
      lambda: _T("test_gpu_vsheet").test_vic_solve_from_the_recorded_vorticity(None, "g7_s2_t257", "mac"), solve=PCG_VIC)
_case("surfturb-whole-call", ["surfturb", "scan"], lambda: _T("test_gpu_surfturb").test_whole_calls_from_the_recorded_states(None, 1))

EXEMPT = {}     # csrc/*.hip files with kernels that no case names, with the reason (at most two)
IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)


def sweep_case():
    """a case that runs the single-launch MIC sweeps, for test_mic_check_reads_after_the_callers_stream"""
    return next(c for c in CASES if c.id == "mic-rows-16x16x16")
