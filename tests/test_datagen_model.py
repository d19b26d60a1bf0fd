"""CPU: the numpy statement of the smoke data-generation plugins (tests/datagen_model.py) against the recorded outputs of the
reference (tests/golden/datagen.npz, written by tools/record_datagen.py): blur, projection, Laplacian and curvature bit for bit, the
centre of mass bit for bit where the reference's fp32 sums are exact and within the derived bound elsewhere."""
import math

import numpy as np
import pytest

import datagen_model as M

f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return np.load(M.GOLDEN)


def test_every_recorded_key_belongs_to_a_case(golden):
    want = set()
    for name, _, _ in M.blur_cases():
        want |= {"blur/%s/real" % name, "blur/%s/mac" % name, "blur/%s/mdim" % name}
    want |= {"com/%s" % n for n in M.COM_CASES}
    want |= {M.project_key(d, m, s) for d in M.PROJECT_DIMS for m in M.PROJECT_MODES for s in M.PROJECT_SCALES} | {"project/const"}
    want |= {key for key, _, _, _ in M.stencil_cases()}
    want |= {"st/iterations", "st/phi", "st/vel", "st/curv"}
    want |= {"dg/iterations", "dg/com", "dg/density", "dg/vel", "dg/xl_density", "dg/img_high", "dg/img_low"}
    assert set(golden.files) == want


def test_recorded_loops(golden):
    C = M.DG_LOOP
    its = golden["dg/iterations"]
    assert its.shape == (C["steps"], 2) and (its[:, 0] > 0).all()
    assert (its[0::C["resetN"], 1] == -1).all() and (its[1::C["resetN"], 1] > 0).all()      # the coarse solver only solves between resets
    assert M.same(M.project(golden["dg/xl_density"], 0, 5.0), golden["dg/img_high"])
    assert M.same(M.project(golden["dg/density"], 0, 5.0), golden["dg/img_low"])
    assert golden["dg/com"].shape == (C["steps"], 3)
    assert golden["st/iterations"].shape == (M.ST_LOOP["steps"],) and (golden["st/iterations"] > 0).all()
    # the recorded curvature is CurvatureOp of the recorded level set (the solve does not touch phi)
    curv = M.curvature(golden["st/phi"], golden["st/curv"], 1.0)
    assert M.same(curv, golden["st/curv"])


@pytest.mark.parametrize("sigma,mdim", M.WEIGHT_SIGMAS)
def test_weights(sigma, mdim):
    n, w = M.weights(sigma)
    assert n == mdim == len(w) and w.dtype == f32
    assert (w == w[::-1]).all() and (w > 0).all() and w[n // 2] == w.max()
    m = f32(1.0 / (math.sqrt(2.0 * math.pi) * float(f32(sigma))))
    assert w[n // 2] == m                                  # exp(-0) = 1: the centre weight is m itself; nothing is normalised


def test_weights_refuse_a_sigma_that_is_not_positive():
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            M.weights(bad)


@pytest.mark.parametrize("name,dims,sigma", M.blur_cases(), ids=[c[0] for c in M.blur_cases()])
def test_blur(golden, name, dims, sigma):
    for ncomp, key in ((1, "real"), (3, "mac")):
        src = M.blur_input(name, ncomp)
        assert M.dims_of(src) == dims
        got, mdim = M.blur(src, sigma)
        assert mdim == int(golden["blur/%s/mdim" % name][0])
        assert M.same(got, golden["blur/%s/%s" % (name, key)]), key


def test_blur_special_values_spread(golden):
    """the NaN cell poisons its (2 r + 1)^3 neighbourhood and nothing else does; +inf and -inf meet in a NaN as well"""
    src = M.blur_input("special", 1)
    got = golden["blur/special/real"]
    r = M.weights(M.BLUR_SPECIAL[1])[0] // 2
    k, j, i = np.argwhere(np.isnan(src))[0]
    assert np.isnan(got[max(k - r, 0):k + r + 1, max(j - r, 0):j + r + 1, max(i - r, 0):i + r + 1]).all()
    assert np.isfinite(got).any() and np.isinf(got).any()


@pytest.mark.parametrize("name", M.COM_CASES)
def test_center_of_mass(golden, name):
    d = M.com_input(name)
    ref = golden["com/%s" % name]
    assert M.same(M.center_of_mass_serial(d), ref)          # the reference's own serial sum, restated
    got = M.center_of_mass(d)
    if name in M.COM_EXACT:
        assert M.same(got, ref)
    else:
        bound = M.com_bound(d, ref)
        for q in range(3):
            err = abs(float(got[q]) - float(ref[q]))
            print(name, "xyz"[q], "contract - reference", err, "bound", bound[q])
            assert err <= bound[q]


def test_center_of_mass_branches():
    assert float(f32(M.com_input("tiny").astype(np.float64).sum())) <= 1e-6 < 2e-6
    assert M.same(M.center_of_mass(M.com_input("zero")), np.zeros(3, f32))
    t = M.com_input("tiny")
    assert M.same(M.center_of_mass(t), np.array([f32(2.0 ** -21) * f32(2.5) + f32(2.0 ** -22) * f32(4.5),
                                                 f32(2.0 ** -21) * f32(3.5) + f32(2.0 ** -22) * f32(1.5), f32(3 * 2.0 ** -23)], f32))


@pytest.mark.parametrize("dims", M.PROJECT_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_projection(golden, dims):
    val = M.project_input(dims)
    sx, sy, sz = dims
    for mode in M.PROJECT_MODES:
        for scale in M.PROJECT_SCALES:
            want = golden[M.project_key(dims, mode, scale)]
            assert want.shape == (max(dims), sx + sz + sx if sz > 1 else sx, 3) and want.dtype == np.uint8
            assert M.same(M.project(val, mode, scale), want), (mode, scale)
    # a shadeMode that is neither 0 nor 1 takes the default arm, smoke
    assert M.same(golden[M.project_key(dims, 3, 1.0)], golden[M.project_key(dims, 0, 1.0)])
    assert not M.same(golden[M.project_key(dims, 1, 1.0)], golden[M.project_key(dims, 0, 1.0)])
    # the clamp and the truncation both act
    img = golden[M.project_key(dims, 0, 4.0)]
    assert img.max() == 255 and 0 < np.unique(img).size


def test_projection_views_add_up():
    val = M.project_input((7, 5, 4))
    full = M.project(val, 0, 1.0)
    parts = [M.project(val, 0, 1.0, views=v) for v in (1, 2, 4)]
    assert M.same(full, parts[0] | parts[1] | parts[2])
    assert all(p.any() for p in parts)


def test_projection_of_a_constant_grid(golden):
    want = golden["project/const"]
    assert M.same(M.project(M.project_const(), 1, 1.0), want)
    assert (M.light(M.project_const()) == 0).all()          # normalize's zero-vector branch


@pytest.mark.parametrize("key,kind,dims,h", M.stencil_cases(), ids=[c[0] for c in M.stencil_cases()])
def test_laplacian_and_curvature(golden, key, kind, dims, h):
    g = M.stencil_input(kind, dims)
    out = np.full(g.shape, M.SENTINEL, f32)
    got = M.laplacian(g, out) if h is None else M.curvature(g, out, h)
    want = golden[key]
    assert M.same(got, want)
    border = np.ones(g.shape, bool)
    border[M._inner(g)] = False
    assert (want[border] == M.SENTINEL).all() and border.sum() > 0
    if kind == "const":
        assert (want[~border] == 0).all()                   # denom at its floor: 0 / pow(1e-6f, 1.5)


def test_one_ulp_measure():
    ref = np.array([1.0, -3.5, 0.0, 1e-45, np.inf], f32)
    ok, nd = M.within_one_ulp(np.nextafter(ref, f32(2)), ref)
    assert not ok and nd == 5                               # next after inf toward 2 is finite: not within a ulp
    ok, nd = M.within_one_ulp(np.nextafter(ref[:4], f32(2)), ref[:4])
    assert ok and nd == 4
    ok, nd = M.within_one_ulp(np.nextafter(np.nextafter(ref[:2], f32(9)), f32(9)), ref[:2])
    assert not ok and nd == 2
