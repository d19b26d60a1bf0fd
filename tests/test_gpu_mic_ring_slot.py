"""-m gpu: the row sweeps of the MIC apply on packed operands keep ONE 16-byte ring slot per cell -- {value -> result, Aprecond, packed
byte, var1} -- and rebuild fluid and the products A * Aprecond from it in the compute and the publisher wave; an unpackable matrix
keeps the coefficient-array layout in the same LDS block.  HIP against the oracle through the C ABI, bit for bit, at the smallest
shapes that reach every way a slot is written, read, reused and published (ring_slot_cases.SHAPES)."""
import numpy as np
import pytest

import cases
import ring_slot_cases as rs
from util import assert_bitexact, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5   # the bar of test_mic_every_sweep_mode for a CG solution (fp64 partial sums combined in another order)


@pytest.mark.parametrize("dims", [s for s, _ in rs.SHAPES])
def test_ring_slot_mic_init_and_apply(hip, oracle, dims):
    for seed in rs.SEEDS:
        flags, A, src = cases.system_inputs(dims, seed)
        assert rs.takes_packed_path(dims, A), (dims, seed)
        ap, dst = cases.run_mic_impl(hip, dims, flags, A, src)
        ap_o, dst_o = cases.run_mic_impl(oracle, dims, flags, A, src)
        assert_bitexact(ap, ap_o, "Aprecond seed %d" % seed)
        assert_bitexact(dst, dst_o, "mic apply seed %d" % seed)


def test_ring_slot_signed_zeros_negative_and_huge_operands(hip, oracle):
    """the operand pattern of test_mic_apply_signed_zeros_negative_and_huge_operands across a ring wrap: the products (+0 | -1) * Aprecond
    are formed from the slot in the compute and the publisher wave, for Aprecond negative, +-0 and denormal and values that are signed
    zeros, denormals or overflow inside the sweep.  NaNs in the same cells, identical bits everywhere else."""
    dims = rs.SIGNED_ZEROS_SHAPE
    sx, sy, sz = dims
    flags, A, src = cases.system_inputs(dims, rs.SIGNED_ZEROS_SEED)
    assert rs.takes_packed_path(dims, A)
    rng = np.random.default_rng(99)
    src = src.copy()
    src[rng.random(src.shape) < 0.15] = 0.0
    src[rng.random(src.shape) < 0.10] = -0.0
    src[rng.random(src.shape) < 0.03] = np.float32(1e-41)
    src[rng.random(src.shape) < 0.002] = np.float32(3e37)
    res = []
    for impl in (hip, oracle):
        f = impl.dev(flags)
        dA = [impl.dev(a) for a in A]
        ap = impl.dev(np.zeros((sz, sy, sx), np.float32))
        impl.call("mf_mic_init", sx, sy, sz, f, ap, dA[0], dA[1], dA[2], dA[3], None)
        impl.sync()
        ap_h = impl.host(ap).copy()
        r2 = np.random.default_rng(5)
        ap_h[r2.random(ap_h.shape) < 0.10] *= np.float32(-1.0)
        ap_h[r2.random(ap_h.shape) < 0.05] = 0.0
        ap_h[r2.random(ap_h.shape) < 0.05] = -0.0
        ap_h[r2.random(ap_h.shape) < 0.02] = np.float32(1e-40)
        ap2 = impl.dev(ap_h)
        dst = impl.dev(np.full((sz, sy, sx), 0.25, np.float32))
        impl.call("mf_mic_apply", sx, sy, sz, f, dst, impl.dev(src), ap2, dA[1], dA[2], dA[3], None)
        impl.sync()
        res.append(impl.host(dst))
    got, want = res
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), "NaNs in different cells: %d vs %d" % (nan_g.sum(), nan_w.sum())
    assert (~nan_w).sum() > 0.2 * want.size
    differ = got[~nan_w].view(np.uint32) != want[~nan_w].view(np.uint32)
    assert not differ.any(), "finite results differ in %d cells" % differ.sum()


def test_ring_slot_unpackable_matrix_keeps_the_array_layout(hip, oracle):
    """one coefficient of -0.5: the sweeps run on the coefficient arrays, whose ring shares its LDS with the slots, across a ring wrap"""
    dims = rs.UNPACKABLE_SHAPE
    flags, A, src = rs.unpackable_system()
    assert not rs.takes_packed_path(dims, A)
    ap, dst = cases.run_mic_impl(hip, dims, flags, A, src)
    ap_o, dst_o = cases.run_mic_impl(oracle, dims, flags, A, src)
    assert_bitexact(ap, ap_o, "Aprecond")
    assert_bitexact(dst, dst_o, "mic apply")


@pytest.mark.parametrize("dims", rs.CG_SHAPES)
def test_ring_slot_cg_solve_fused_dot(hip, oracle, dims):
    """mf_cg_solve with the MIC preconditioner: the backward sweep's fused dot(dst, var1) takes var1 from the slot"""
    flags, A, _ = cases.system_inputs(dims, rs.CG_SEED)
    assert rs.takes_packed_path(dims, A)
    rhs = cases.cg_rhs(dims, flags, rs.CG_SEED)
    xo, sto = cases.run_cg_impl(oracle, dims, flags, A, rhs, 2, 1e-4, 50, 0)
    x, st = cases.run_cg_impl(hip, dims, flags, A, rhs, 2, 1e-4, 50, 0)
    assert st[0] == sto[0], (st, sto)
    e = rel_err(x, xo)
    assert e <= TOL, "cg solution: relative error %g > %g" % (e, TOL)
