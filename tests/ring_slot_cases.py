"""Inputs of the MIC ring-slot tests (tests/test_gpu_mic_ring_slot.py on the GPU, tests/test_mic_ring_slot_inputs.py without one):
the smallest shapes at which the 16-byte operand slots of the row sweeps' packed path (k_mic_rows) can go wrong, and the host-side
statement of the condition under which the library takes that path."""
import numpy as np

import cases

# 8 x 8 rows per bundle, 8 cells per chunk, a ring of 64 steps = 8 chunks
SHAPES = [
    ((8, 8, 8), "one bundle, one chunk: edge blocks only"),
    ((16, 9, 9), "2 x 2 bundles with rows outside the grid (their slots must hold neutral values), faces in both directions"),
    ((72, 8, 8), "9 chunks > ring / 8: a slot is reused after write-back and publish"),
    ((136, 17, 8), "two ring wraps, a j hop into a bundle with outside rows (17 chunks would also wrap a 128-step ring)"),
    ((72, 8, 24), "k hops with ring wrap"),
]
SEEDS = (1, 2)
SIGNED_ZEROS_SHAPE = (72, 16, 8)
SIGNED_ZEROS_SEED = 7
UNPACKABLE_SHAPE = (72, 9, 8)
UNPACKABLE_SEED = 5
CG_SHAPES = [(72, 16, 16), (136, 17, 8)]
CG_SEED = 3

MINUS_ONE = np.float32(-1.0).view(np.uint32)


def takes_packed_path(dims, A):
    """what mf_mic_init certifies before the sweeps run on packed bytes: whole chunks of 8 cells per row, and every Ai / Aj / Ak
    entry exactly +0 or -1 (bit patterns: -0 does not qualify)"""
    if dims[0] % 8 != 0:
        return False
    for a in A[1:4]:
        bits = np.ascontiguousarray(a, np.float32).view(np.uint32)
        if not np.all((bits == 0) | (bits == MINUS_ONE)):
            return False
    return True


def unpackable_system(dims=UNPACKABLE_SHAPE, seed=UNPACKABLE_SEED):
    """a Laplace system with one Aj coefficient set to -0.5 (as test_mic_and_cg_with_a_matrix_that_cannot_be_packed's "one_cell")"""
    flags, A, src = cases.system_inputs(dims, seed)
    A = [a.copy() for a in A]
    nz = np.argwhere(A[2] != 0)
    kk, jj, ii = nz[len(nz) // 2]
    A[2][kk, jj, ii] = np.float32(-0.5)
    return flags, A, src
