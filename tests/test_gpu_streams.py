"""-m gpu: every kernel family on a caller's non-blocking stream (tests/stream_cases.py has the helpers, the case table and the reasons).

include/manta_hip.h promises that every entry works on the caller's stream.  The rest of the suite only ever uses the default (null)
stream, where library work that ignores the stream argument is still ordered by accident.  Here the package and the raw entries run
inside a torch side stream, which does not wait for the null stream and which the null stream does not wait for:

  * with the default stream idle (every case, the solves included);
  * with the default stream busy for longer than the case takes, so that anything the library puts on the null stream arrives after
    the case's own kernels (every case that runs no MIC sweep and no PCG: those must not run beside other long-running work);
  * raw entries whose inputs reach their argument tensors only by copies queued on the caller's stream behind a busy chain;
  * mf_mic_check after a sweep on the side stream.

The expected values are the oracle's, the numpy models' or the golden files', at the bar of each family's own test."""
import ctypes
import gc
import math

import numpy as np
import pytest
import torch

import cases
import stream_cases as S
import util
from util import assert_bitexact

pytestmark = pytest.mark.gpu

LATE = [c for c in S.CASES if not c.solve]


@pytest.mark.parametrize("case", S.CASES, ids=S.IDS)
def test_family_on_side_stream(hip_backend, case):
    torch.cuda.synchronize()                    # the default stream is idle
    with S.poisoned_pools(), S.side_stream():
        case.check(case.run())


@pytest.mark.parametrize("case", LATE, ids=[c.id for c in LATE])
def test_family_on_side_stream_while_default_stream_is_late(hip_backend, case):
    beside = S.stream_beside_default()
    with S.poisoned_pools():
        with S.side_stream(beside):
            case.run()      # first use is behind us: growing an arena or making the device's workspace synchronises the device, once
        gc.collect()        # solvers are reference cycles; one that owns a multigrid hierarchy calls mf_mg_destroy (a device-wide wait) when collected
        ev = S.busy(torch.cuda.default_stream(), S.SPAN)
        try:
            with S.side_stream(beside):
                got = case.run()
                chain_still_running = not ev.query()
                case.check(got)
            assert chain_still_running or case.device_syncs, "busy chain too short"
        finally:
            ev.synchronize()


# ---- raw entries whose inputs arrive through stream order alone ------------------------------------------------------------------------
RAW_DIMS = [(16, 12, 10), (33, 17, 9)]
RAW_ENTRIES = ["mf_apply_matrix", "mf_semi_lagrange_real", "mf_grid_dot", "mf_grid_max_abs", "mf_interpolate_grid", "mf_shape_levelset"]
HOST_SCALAR = ("mf_grid_dot", "mf_grid_max_abs")


def _raw_inputs(entry, dims):
    """-> (numpy inputs by name, output shape or None)"""
    sx, sy, sz = dims
    shape = (sz, sy, sx)
    if entry == "mf_apply_matrix":
        flags, A, src = cases.system_inputs(dims, 3)
        return dict(flags=flags, src=src, A0=A[0], Ai=A[1], Aj=A[2], Ak=A[3]), shape
    if entry == "mf_semi_lagrange_real":
        return dict(vel=util.rand_vel(sx, sy, sz, 41, 2.5), src=util.rand_real(shape, 42)), shape
    if entry == "mf_grid_dot":
        return dict(a=util.rand_real(shape, 43, 3.0), b=util.rand_real(shape, 44, 2.0)), None
    if entry == "mf_grid_max_abs":
        return dict(a=util.rand_real(shape, 45, 3.0)), None
    if entry == "mf_interpolate_grid":
        return dict(source=util.rand_real(((sz + 1) // 2, (sy + 1) // 2, (sx + 1) // 2), 46)), shape
    return {}, shape


def _raw_call(impl, entry, dims, t, out, stream):
    """one call of the entry on implementation `impl` with the argument tensors t; -> the host scalar, if the entry has one"""
    sx, sy, sz = dims
    n = sx * sy * sz
    if entry == "mf_apply_matrix":
        impl.call(entry, sx, sy, sz, t["flags"], out, t["src"], t["A0"], t["Ai"], t["Aj"], t["Ak"], stream)
    elif entry == "mf_semi_lagrange_real":
        impl.call(entry, sx, sy, sz, t["vel"], out, t["src"], 0.9, 1, 1, stream)       # orderTrace 1, linear: the z-marching kernel
    elif entry == "mf_grid_dot":
        r = ctypes.c_double(float("nan"))
        impl.call(entry, n, t["a"], t["b"], ctypes.byref(r), stream)
        return r.value
    elif entry == "mf_grid_max_abs":
        r = ctypes.c_float(float("nan"))
        impl.call(entry, n, t["a"], ctypes.byref(r), stream)
        return r.value
    elif entry == "mf_interpolate_grid":
        ssx, ssy, ssz = (sx + 1) // 2, (sy + 1) // 2, (sz + 1) // 2
        f = [float(np.float32(a) / np.float32(b)) for a, b in ((ssx, sx), (ssy, sy), (ssz, sz))]
        impl.call(entry, sx, sy, sz, out, ssx, ssy, ssz, t["source"], 1, f[0], f[1], f[2], 0.0, 0.0, 0.0, 1, stream)
    else:
        q = (ctypes.c_float * 12)(*[float(np.float32(v)) for v in (sx * 0.5, sy * 0.4, sz * 0.5, sx * 0.27, 1.0, 1.0, 1.0, 0, 0, 0, 0, 0)])
        impl.call(entry, sx, sy, sz, 1, q, out, stream)


@pytest.mark.parametrize("dims", RAW_DIMS, ids=lambda d: "%dx%dx%d" % d)
@pytest.mark.parametrize("entry", RAW_ENTRIES)
def test_raw_entries_when_their_own_stream_is_late(hip, oracle, entry, dims):
    inputs, out_shape = _raw_inputs(entry, dims)
    staging = {k: hip.dev(v) for k, v in inputs.items()}
    torch.cuda.synchronize()
    S_ = torch.cuda.Stream()
    with torch.cuda.stream(S_):
        args = {k: torch.full_like(v, 0x7f7f7f7f if v.dtype == torch.int32 else float("nan")) for k, v in staging.items()}
        out = None if out_shape is None else torch.full(out_shape, float("nan"), dtype=torch.float32, device="cuda")
        S.busy(S_, S.SPAN)
        for k in args:
            args[k].copy_(staging[k])           # device to device, queued behind the chain
        value = _raw_call(hip, entry, dims, args, out, ctypes.c_void_p(S_.cuda_stream))
        if entry in HOST_SCALAR:
            assert S_.query(), "an entry that returns through a host pointer synchronises the stream"
        S_.synchronize()
        got = None if out is None else out.cpu().numpy()
    if entry == "mf_grid_dot":
        want = math.fsum((inputs["a"].reshape(-1) * inputs["b"].reshape(-1)).astype(np.float64))      # fp32 products, their exact sum rounded once
        assert abs(value - want) <= 1e-12 * abs(want) and np.float32(value) == np.float32(want), (value, want)
    elif entry == "mf_grid_max_abs":
        assert value == float(np.abs(inputs["a"]).max()), value
    else:
        o_out = oracle.dev(np.full(out_shape, np.nan, np.float32))
        _raw_call(oracle, entry, dims, {k: oracle.dev(v) for k, v in inputs.items()}, o_out, None)
        assert_bitexact(got, oracle.host(o_out), entry)


def test_mic_check_reads_after_the_callers_stream(hip_backend):
    """mf_mic_check on the stream the sweeps ran on: it waits for that stream, then reads the flag the sweeps latch on the device"""
    case = S.sweep_case()
    with S.side_stream() as st:
        case.check(case.run())
        assert S.simpl().lib.cdll.mf_mic_check(ctypes.c_void_p(st.cuda_stream)) == 0
