"""tests/reduce_model.py against independent statements: the exactly rounded sum, numpy's extremes, and the centre-of-mass function it
replaced (kept here verbatim as the yardstick)."""
import math

import numpy as np
import pytest

import datagen_model as D
import reduce_model as R

f32, f64 = np.float32, np.float64
RULES = [(2048, 1024), (1024, 2048), (256, None)]        # (items per block, block cap) of the call sites
SIZES = [1, 255, 2048, 2049, 257 * 2048 + 5, 1024 * 2048 + 2049]


def values(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f32)


def datagen_fixed_order_sum(t):
    """tests/datagen_model.fixed_order_sum as it stood before reduce_model"""
    def wave_sum(v):
        for o in (32, 16, 8, 4, 2, 1):
            v = v[..., :o] + v[..., o:2 * o]
        return v[..., 0]

    def block_sum(v):
        w = wave_sum(v.reshape(v.shape[:-1] + (4, 64)))
        return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]

    t = np.asarray(t, f64)
    n = t.size
    nb = min(max((n + 1023) // 1024, 1), 2048)
    T = nb * 256
    rows = (n + T - 1) // T
    p = np.zeros(rows * T, f64)
    p[:n] = t
    p = p.reshape(rows, T)
    live = (np.arange(rows * T) < n).reshape(rows, T)
    acc = np.zeros(T, f64)
    for r in range(rows):
        acc = np.where(live[r], acc + p[r], acc)
    part = block_sum(acc.reshape(nb, 256))
    rows2 = (nb + 255) // 256
    q = np.zeros(rows2 * 256, f64)
    q[:nb] = part
    q = q.reshape(rows2, 256)
    live2 = (np.arange(rows2 * 256) < nb).reshape(rows2, 256)
    acc2 = np.zeros(256, f64)
    for r in range(rows2):
        acc2 = np.where(live2[r], acc2 + q[r], acc2)
    return float(block_sum(acc2))


@pytest.mark.parametrize("rule", RULES, ids=str)
@pytest.mark.parametrize("n", SIZES)
def test_sum_against_fsum(n, rule):
    """any order of n fp64 additions lies within n 2^-53 sum |t| of the exact sum"""
    t = values(n, n % 1000).astype(f64)
    got = R.fixed_order_sum(t, *rule)
    want = math.fsum(t.tolist())
    bound = n * 2.0 ** -53 * math.fsum(np.abs(t).tolist())
    print(n, rule, "model - fsum", abs(got - want), "bound", bound)
    assert abs(got - want) <= bound


def test_sum_depends_on_the_rule():
    """the inputs tell one tree from another: the three rules give three sums"""
    t = values(257 * 2048 + 5, 5)
    assert len({R.fixed_order_sum(t, *rule) for rule in RULES}) == 3


@pytest.mark.parametrize("name", D.COM_CASES)
def test_sum_reproduces_datagen(name):
    for t in D.com_terms(D.com_input(name)):
        assert R.fixed_order_sum(t) == datagen_fixed_order_sum(t)
        assert R.fixed_order_sum(t, 1024, 2048) == datagen_fixed_order_sum(t)


@pytest.mark.parametrize("n", [1024 * 1024 + 1, 2048 * 1024 + 77])
def test_sum_reproduces_datagen_past_one_block(n):
    t = values(n, 3)
    assert R.fixed_order_sum(t) == datagen_fixed_order_sum(t)


@pytest.mark.parametrize("rule", RULES, ids=str)
@pytest.mark.parametrize("n", SIZES)
def test_min_max(n, rule):
    a = values(n, 40 + n % 7)
    lo, hi = R.fixed_order_min_max(a, *rule)
    assert (lo, hi) == (a.min(), a.max()) and lo.dtype == f32
    a[::3] = np.nan                                     # a NaN loses against a number; all NaN: the identities
    b = a[~np.isnan(a)]
    assert R.fixed_order_min_max(a, *rule) == ((b.min(), b.max()) if len(b) else (R.FLT_MAX, -R.FLT_MAX))
    i = np.random.default_rng(n).integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    assert R.fixed_order_min_max(i, *rule) == (i.min(), i.max())
    d = np.abs(values(n, 9)).astype(f64)
    assert R.fixed_order_max(d, *rule) == d.max()
    assert R.fixed_order_max(np.full(n, np.nan), *rule) == 0.0


def test_signed_zeros():
    """-0 is below +0 on either side"""
    z, nz = f32(0.0), f32(-0.0)
    for a, b in ((z, nz), (nz, z)):
        assert np.signbit(R.fmin(a, b)) and not np.signbit(R.fmax(a, b))
    assert np.signbit(R.fmax(nz, nz)) and not np.signbit(R.fmin(z, z))
    v = np.abs(values(3000, 1))
    v[::5], v[2::7] = z, nz
    lo, hi = R.fixed_order_min_max(v)
    assert lo == 0 and np.signbit(lo) and hi == v.max()
    lo, hi = R.fixed_order_min_max(-v)
    assert hi == 0 and not np.signbit(hi) and lo == -v.max()
