"""The fixed tree of the library's two-stage device reduction (mantaflow_amd/csrc/reduce.h), restated in numpy.

nb = min(max(ceil(n / per_block), 1), cap) blocks of 256 threads; thread g of the grid folds items g, g + 256 nb, ... in order; each block
folds its 256 accumulators (six shuffle-down steps per 64-lane wave, then the four wave results in order); one finishing block whose
thread q folds partials q, q + 256, ... in order, then the same block fold.  The accumulator is always the left operand.

The two parameters that differ between the call sites are per_block and cap: 2048 / 1024 at most sites, 1024 / 2048 for the centre of
mass, primal-dual guiding and the plain MIC dot, 256 / None (one item per thread, no cap) for the mesh volume."""
import numpy as np

f32, f64 = np.float32, np.float64
FLT_MAX = f32(np.finfo(np.float32).max)


def blocks_for(n, per_block, cap):
    nb = max((n + per_block - 1) // per_block, 1)
    return nb if cap is None else min(nb, cap)


def _wave_fold(v, op):
    """lane 0 of the 64-lane shuffle-down reduction (offsets 32, 16, .. 1) along the last axis"""
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v[..., :o], v[..., o:2 * o])
    return v[..., 0]


def _block_fold(v, op):
    """thread 0 of a 256-thread block fold along the last axis: the four wave results folded in order"""
    w = _wave_fold(v.reshape(v.shape[:-1] + (4, 64)), op)
    return op(op(op(w[..., 0], w[..., 1]), w[..., 2]), w[..., 3])


def _strided_fold(t, T, op, identity):
    """accumulator g of T folds t[g], t[g + T], ... in order, starting from the identity"""
    n = t.size
    rows = max((n + T - 1) // T, 1)
    p = np.full(rows * T, identity, t.dtype)
    p[:n] = t
    p = p.reshape(rows, T)
    live = (np.arange(rows * T) < n).reshape(rows, T)
    acc = np.full(T, identity, t.dtype)
    for r in range(rows):
        acc = np.where(live[r], op(acc, p[r]), acc)
    return acc


def fixed_order_fold(t, op, identity, per_block, cap):
    t = np.asarray(t).ravel()
    nb = blocks_for(t.size, per_block, cap)
    part = _block_fold(_strided_fold(t, nb * 256, op, identity).reshape(nb, 256), op)
    return _block_fold(_strided_fold(part, 256, op, identity), op)


def _wave_sum(v):
    return _wave_fold(v, np.add)


def _block_sum(v):
    return _block_fold(v, np.add)


def fixed_order_sum(t, per_block=1024, cap=2048):
    """the fp64 sum of the terms t (fp32 or fp64 values, converted exactly) in the library's order"""
    return float(fixed_order_fold(np.asarray(t, f64), np.add, f64(0), per_block, cap))


# fminf / fmaxf as the gfx9 v_min_f32 / v_max_f32 evaluate them (the ISA's pseudo-code, IEEE 754-2019 minimumNumber): a NaN operand
# loses against a number, and -0 is below +0 whichever side it stands on
def fmin(a, b):
    a, b = np.asarray(a), np.asarray(b)
    r = np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(b < a, b, a)))
    zeros = (a == 0) & (b == 0)
    return np.where(zeros & (np.signbit(a) | np.signbit(b)), -np.zeros_like(r), r).astype(a.dtype)


def fmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    r = np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(b > a, b, a)))
    zeros = (a == 0) & (b == 0)
    return np.where(zeros & ~(np.signbit(a) & np.signbit(b)), np.zeros_like(r), r).astype(a.dtype)


def fixed_order_min_max(t, per_block=2048, cap=1024):
    """(min, max) of the fp32 values t, from +-FLT_MAX, or of int32 values, from INT32_MAX / INT32_MIN, in the library's order"""
    t = np.asarray(t).ravel()
    if t.dtype.kind == "i":
        t = t.astype(np.int32)
        info = np.iinfo(np.int32)
        return (np.int32(fixed_order_fold(t, np.minimum, np.int32(info.max), per_block, cap)),
                np.int32(fixed_order_fold(t, np.maximum, np.int32(info.min), per_block, cap)))
    t = t.astype(f32)
    return f32(fixed_order_fold(t, fmin, FLT_MAX, per_block, cap)), f32(fixed_order_fold(t, fmax, -FLT_MAX, per_block, cap))


def fixed_order_max(t, per_block=2048, cap=1024):
    """the fp64 maximum of the non-negative values t, from 0, in the library's order"""
    return float(fixed_order_fold(np.asarray(t, f64), fmax, f64(0), per_block, cap))
