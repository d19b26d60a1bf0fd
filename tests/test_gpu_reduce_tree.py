"""The shared two-stage reduction (mantaflow_amd/csrc/reduce.h) through public entries, one group per fold, bit for bit against
tests/reduce_model.py.  Sizes: one item; one block exactly and a second block with one item (2048 items per block); the finisher's
threads take a second partial; the block cap is reached and the grid's threads wrap with a ragged tail.  The K = 4 fold (calcCenterOfMass)
is pinned in test_gpu_datagen.py."""
import ctypes

import numpy as np
import pytest

import reduce_model as R

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SIZES = [1, 2048, 2049, 257 * 2048 + 5, 1024 * 2048 + 2049]
NMAX = max(SIZES)
FLUID = 1


def _values(seed):
    """mixed signs and magnitudes over six decades: a sum in another order differs in the low bits"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, NMAX) * 10.0 ** rng.uniform(-3, 3, NMAX)).astype(f32)


@pytest.fixture(scope="module")
def data(hip):
    h = {"a": _values(11), "b": _values(12)}
    rng = np.random.default_rng(13)
    h["flags"] = np.where(rng.random(NMAX) < 0.7, FLUID, 4).astype(np.int32)
    h["ia"] = rng.integers(-2 ** 31, 2 ** 31, NMAX, dtype=np.int64).astype(np.int32)
    return h, {k: hip.dev(v) for k, v in h.items()}


def bits(x):
    return np.asarray(x).tobytes()


def shape2d(n):
    """(sx, sy) with sx * sy == n and sx >= 3 where n has such a factor (a 2-D grid needs an interior column)"""
    for sx in range(3, 64):
        if n % sx == 0 and n // sx >= 2:
            return sx, n // sx
    raise AssertionError(n)


@pytest.mark.parametrize("n", SIZES)
def test_sum_f64(hip, data, n):
    h, d = data
    a, b = h["a"][:n], h["b"][:n]
    r = ctypes.c_double(-1.0)
    hip.call("mf_grid_dot", n, d["a"], d["b"], ctypes.byref(r), None)
    want = R.fixed_order_sum(a * b, 2048, 1024)
    print("mf_grid_dot", n, repr(r.value), repr(want))
    assert bits(f64(r.value)) == bits(f64(want))
    hip.call("mf_grid_sum_sqr", n, d["a"], ctypes.byref(r), None)
    want = R.fixed_order_sum(a.astype(f64) * a.astype(f64), 2048, 1024)
    print("mf_grid_sum_sqr", n, repr(r.value), repr(want))
    assert bits(f64(r.value)) == bits(f64(want))

    # getGridAvg: the sum and the count of the fluid cells, two values folded together
    fl = h["flags"][:n] == FLUID
    g = ctypes.c_float(-2.0)
    hip.call("mf_gridops_grid_avg", n, d["a"], d["flags"], ctypes.byref(g), None)
    s, cnt = R.fixed_order_sum(np.where(fl, a, f32(0)), 2048, 1024), R.fixed_order_sum(fl.astype(f64), 2048, 1024)
    assert cnt == fl.sum()
    want = f32(s * (1. / cnt)) if cnt > 0 else f32(-1)
    print("getGridAvg", n, repr(g.value), repr(want))
    assert bits(f32(g.value)) == bits(want)

    # getL1 / getL2 of a Real grid and totalSum: a grid has at least 2 x 2 cells, so one item is the interior of a 3 x 3 grid (bnd = 1)
    # for the norms and out of reach for totalSum, whose reduction runs over all cells and skips the boundary
    sx, sy, bnd = (3, 3, 1) if n == 1 else shape2d(n) + (0,)
    cells = h["a"][:sx * sy].reshape(sy, sx)
    inner = cells[bnd:sy - bnd, bnd:sx - bnd].ravel()
    for l2 in (0, 1):
        hip.call("mf_gridops_norm", 0, l2, sx, sy, 1, bnd, d["a"], ctypes.byref(g), None)
        acc = R.fixed_order_sum(inner * inner if l2 else np.abs(inner), 2048, 1024)
        want = f32(np.sqrt(f64(acc))) if l2 else f32(acc)
        print("getL%d" % (l2 + 1), n, repr(g.value), repr(want))
        assert bits(f32(g.value)) == bits(want)
    if n > 1:
        interior = np.zeros((sy, sx), bool)
        interior[1:-1, 1:-1] = True
        hip.call("mf_fields_total_sum", sx, sy, 1, d["a"], ctypes.byref(g), None)
        want = f32(R.fixed_order_sum(np.where(interior, cells, f32(0)), 2048, 1024))
        print("totalSum", n, repr(g.value), repr(want))
        assert bits(f32(g.value)) == bits(want)


def zero_extremes(a, sign):
    """sign * |a| with +0 and -0 sprinkled in: the extreme towards zero is a zero, and its sign is the fold's to decide"""
    v = (f32(sign) * np.abs(a)).astype(f32)
    v[::5] = f32(0.0)
    v[2::7] = f32(-0.0)
    return v


@pytest.mark.parametrize("case", ["mixed", "zero-min", "zero-max"])
@pytest.mark.parametrize("n", SIZES)
def test_min_max_f32(hip, data, n, case):
    h, d = data
    a, dev = h["a"][:n], d["a"]
    if case != "mixed":
        a = zero_extremes(a, 1 if case == "zero-min" else -1)
        dev = hip.dev(a)
    lo, hi = ctypes.c_float(5.0), ctypes.c_float(5.0)
    hip.call("mf_grid_min_max", n, dev, ctypes.byref(lo), ctypes.byref(hi), None)
    wlo, whi = R.fixed_order_min_max(a, 2048, 1024)
    print("mf_grid_min_max", n, case, repr(lo.value), repr(hi.value), repr(wlo), repr(whi))
    assert bits(f32(lo.value)) == bits(wlo) and bits(f32(hi.value)) == bits(whi)
    out = hip.dev(np.full(1, -1.0, f64))
    hip.call("mf_grid_max_abs_dev_f64", n, dev, out, None)
    alo, ahi = abs(wlo), abs(whi)
    assert bits(hip.host(out)[0]) == bits(f64(alo if alo > ahi else ahi))


@pytest.mark.parametrize("n", SIZES)
def test_min_max_i32(hip, data, n):
    h, d = data
    lo, hi = ctypes.c_int32(5), ctypes.c_int32(5)
    hip.call("mf_grid4d_int_min_max", n, d["ia"], ctypes.byref(lo), ctypes.byref(hi), None)
    wlo, whi = R.fixed_order_min_max(h["ia"][:n], 2048, 1024)
    assert (lo.value, hi.value) == (int(wlo), int(whi))


@pytest.mark.parametrize("n", SIZES)
def test_max_f64(hip, data, n):
    h, d = data
    r = ctypes.c_double(-1.0)
    hip.call("mf_grid4d_max_diff", 1, 0, n, d["a"], d["b"], ctypes.byref(r), None)
    want = R.fixed_order_max(np.abs(h["a"][:n] - h["b"][:n]).astype(f64), 2048, 1024)     # grid4dMaxDiff: |a - b| in fp32, widened
    print("mf_grid4d_max_diff", n, repr(r.value), repr(want))
    assert bits(f64(r.value)) == bits(f64(want))
