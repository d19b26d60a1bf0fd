"""No GPU needed: the inputs of tests/test_gpu_mic_ring_slot.py reach the code they are meant for.  The row sweeps run on packed
operands (one 16-byte ring slot per cell) exactly when sx % 8 == 0 and every off-diagonal is +0 or -1; every listed shape and seed
must satisfy that, and the unpackable system must not."""
import numpy as np
import pytest

import cases
import ring_slot_cases as rs


@pytest.mark.parametrize("dims", [s for s, _ in rs.SHAPES])
def test_ring_slot_shapes_take_the_packed_path(dims):
    for seed in rs.SEEDS:
        flags, A, src = cases.system_inputs(dims, seed)
        assert rs.takes_packed_path(dims, A), (dims, seed)
        assert src.shape == (dims[2], dims[1], dims[0])


def test_ring_slot_shapes_reach_what_they_are_listed_for():
    ring_chunks = 8                                   # a 64-step ring holds 8 chunks of 8 cells
    shapes = [s for s, _ in rs.SHAPES]
    bundles = lambda n: (n + 7) // 8
    assert any(sx == 8 and bundles(sy) == 1 and bundles(sz) == 1 for sx, sy, sz in shapes)                       # one bundle, one chunk
    assert any(bundles(sy) > 1 and bundles(sz) > 1 and sy % 8 and sz % 8 for sx, sy, sz in shapes)               # rows outside, both faces
    assert any(ring_chunks < sx // 8 <= 2 * ring_chunks for sx, sy, sz in shapes)                                # a slot is reused once
    assert any(sx // 8 > 2 * ring_chunks and bundles(sy) > 1 and sy % 8 for sx, sy, sz in shapes)                # two wraps, j hop, outside rows
    assert any(sx // 8 > ring_chunks and bundles(sz) > 2 for sx, sy, sz in shapes)                               # k hops with ring wrap


def test_ring_slot_solver_and_special_operand_inputs_take_the_packed_path():
    for dims in rs.CG_SHAPES:
        flags, A, _ = cases.system_inputs(dims, rs.CG_SEED)
        assert rs.takes_packed_path(dims, A), dims
        assert dims[0] // 8 > 8
    flags, A, _ = cases.system_inputs(rs.SIGNED_ZEROS_SHAPE, rs.SIGNED_ZEROS_SEED)
    assert rs.takes_packed_path(rs.SIGNED_ZEROS_SHAPE, A)


def test_ring_slot_unpackable_system_does_not():
    flags, A, _ = rs.unpackable_system()
    assert rs.UNPACKABLE_SHAPE[0] % 8 == 0 and rs.UNPACKABLE_SHAPE[0] // 8 > 8      # only the coefficient keeps it off the packed path
    assert not rs.takes_packed_path(rs.UNPACKABLE_SHAPE, A)
    assert np.count_nonzero(A[2] == np.float32(-0.5)) == 1
    # -0 is not +0: a matrix with a negative zero is refused as well
    B = [a.copy() for a in A]
    B[2][A[2] == np.float32(-0.5)] = np.float32(-1.0)
    assert rs.takes_packed_path(rs.UNPACKABLE_SHAPE, B)
    B[3][B[3] == 0] = np.float32(-0.0)
    assert not rs.takes_packed_path(rs.UNPACKABLE_SHAPE, B)
