"""CPU: the numpy model of the 4-D grids (tests/grid4d_model.py) against the fixture recorded from the compiled reference
(tests/golden/grid4d.npz), bit for bit, for every operation and element type -- and the properties each case exists for, read from the
model's branch counters."""
import os

import numpy as np
import pytest

import grid4d_model as M

f32 = np.float32
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid4d.npz"))


def test_fixture_is_small_and_holds_every_case():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid4d.npz")
    assert os.path.getsize(path) < 500000
    keys = {k.split("#")[0] for k in GOLDEN.files}
    for key, *_ in M.op_cases():
        assert key in keys, key
    for k in GOLDEN.files:                      # what is kept in full is small; what is not is a digest
        assert k.endswith("#sha") or GOLDEN[k].size <= M.FULL_LIMIT or GOLDEN[k].dtype.kind == "U" or k.startswith(("addparts/", "symsha/", "loop2005/", "loop2065/")), k      # the loops are compared within bounds: kept in full


@pytest.mark.parametrize("kind", M.KINDS)
def test_operators_reductions_and_boundaries_equal_the_reference(kind):
    cnt, n = {}, 0
    for key, name, dims, k, op, arg in M.op_cases():
        if k != kind:
            continue
        msg = M.same_as_fixture(GOLDEN, key, M.run_op(dims, kind, op, arg, cnt))
        assert msg is None, msg
        n += 1
    assert n == len(M.SHAPES) * (len(M.ELEMENTWISE) + len(M.REDUCTIONS) + len(M.BOUND_WIDTHS)) + len(M.NEUMANN)
    assert cnt["bound_cells"] > 0 and cnt["inner_cells"] > 0
    for q in range(5):                          # cells out of range on 0 .. 4 axes at once
        assert cnt["neumann_axes_%d" % q] > 0, q


def test_set_bound_widths():
    """w = 0 is the outer layer, w = 1 two layers; at 3^4 every cell is a boundary cell already for w = 1; w = 2 covers 6^4"""
    for w, inner in ((0, (5 * 3 * 2 * 1)), (1, 3 * 1 * 0 * 0), (2, 0)):
        assert int((~M.bound_mask(M.SHAPES["a"], w)).sum()) == inner
    assert M.bound_mask(M.SHAPES["e"], 1).all() and not M.bound_mask(M.SHAPES["e"], 0).all()
    assert M.bound_mask(M.SHAPES["b"], 2).all() and not M.bound_mask(M.SHAPES["b"], 1).all()


def test_set_bound_neumann_precondition_and_map():
    for name, (dims, w) in M.NEUMANN.items():
        assert min(dims) >= 2 * w + 3, name
    with pytest.raises(AssertionError):
        M.set_bound_neumann(M.rand_grid((5, 5, 5, 4), "real", "a"), (5, 5, 5, 4), 1)
    dims, w = M.NEUMANN["n3"]
    a = M.rand_grid(dims, "real", "a")
    out = M.set_bound_neumann(a, dims, w)
    assert out[0, 0, 0, 0] == a[3, 3, 3, 3] and out[6, 6, 6, 8] == a[3, 3, 3, 5]       # corners take the nearest inner corner
    assert out[3, 3, 3, 4] == a[3, 3, 3, 4] and out[3, 3, 3, 2] == a[3, 3, 3, 3]
    assert np.array_equal(out[3, 3, 3, 3:6], a[3, 3, 3, 3:6])                          # inner cells keep their values


def test_regions_slices_and_components_equal_the_reference():
    cnt = {}
    dims = M.SHAPES["a"]
    cells = {}
    for rname, (start, end) in M.REGIONS.items():
        for kind in ("real", "vec4"):
            c = {}
            msg = M.same_as_fixture(GOLDEN, "region/%s/%s" % (rname, kind),
                                    M.set_region(M.rand_grid(dims, kind, "a"), dims, start, end, M.REGION_VALUE[kind], c))
            assert msg is None, msg
            cells[rname] = c["region_cells"]
    # fractional bounds: 1.5 <= i <= 4.25 is i in {2, 3, 4}, 0.5 <= k <= 2.5 is k in {1, 2}, t == 1, all four j
    assert cells == {"frac": 3 * 4 * 2 * 1, "all": int(np.prod(dims)), "none": 0}
    for sname, (shape, srct, dd) in M.SLICES.items():
        sd = M.SHAPES[shape]
        dsh = (dd[2], dd[1], dd[0])
        for kind in ("real", "vec4"):
            src = M.rand_grid(sd, kind, "a")
            r = np.random.default_rng(M._seed("slice", sname, kind))
            dst = r.uniform(-9, 9, dsh + ((3,) if kind == "vec4" else ())).astype(f32)
            dstt = r.uniform(-9, 9, dsh).astype(f32) if kind == "vec4" else None
            for with_t in ((False, True) if kind == "vec4" else (False,)):
                md, mt = M.get_slice(src, srct, dst, dstt if with_t else None, cnt)
                key = "slice/%s/%s%s" % (sname, kind, "/t" if with_t else "")
                msg = M.same_as_fixture(GOLDEN, key, md)
                assert msg is None, msg
                if with_t:
                    msg = M.same_as_fixture(GOLDEN, key + "/dstt", mt)
                    assert msg is None, msg
                if sname in ("below", "above"):                 # an srct outside the grid changes nothing
                    assert np.array_equal(md, dst)
                if sname == "larger":                           # cells the source does not have keep their values
                    assert np.array_equal(md[4:], dst[4:]) and not np.array_equal(md[:4, :5, :7], dst[:4, :5, :7])
    assert cnt["slice_out_of_range"] == 6 and cnt["slice_smaller_dst"] == 3
    for shape in ("a", "c"):
        sd = M.SHAPES[shape]
        v, r = M.rand_grid(sd, "vec4", "a"), M.rand_grid(sd, "real", "b")
        for c in range(4):
            msg = M.same_as_fixture(GOLDEN, "getComp/%s/%d" % (shape, c), M.get_comp(v, c))
            assert msg is None, msg
            msg = M.same_as_fixture(GOLDEN, "setComp/%s/%d" % (shape, c), M.set_comp(r, v, c))
            assert msg is None, msg


@pytest.mark.parametrize("kind", ("real", "vec4"))
def test_interpolation_equals_the_reference(kind):
    cnt = {}
    src = M.rand_grid(M.INTERP_CHAIN[0][1], kind, "chain")
    for name, sd, td in M.INTERP_CHAIN:                 # the chain of test_0042_interpol4d.py at res = 8: 4^4 -> 8^4 -> 16^4 -> 8^4 -> 4^4
        assert M.shape_of(sd, kind) == src.shape
        src = M.interpolate(src, td, cnt=cnt)
        msg = M.same_as_fixture(GOLDEN, "interp/%s/%s" % (name, kind), src)
        assert msg is None, msg
    for name, (sd, td, kw) in M.INTERP_CASES.items():
        c = {}
        msg = M.same_as_fixture(GOLDEN, "interp/%s/%s" % (name, kind), M.interpolate(M.rand_grid(sd, kind, "interp"), td, cnt=c, **kw))
        assert msg is None, msg
        if name == "centre":        # factor 1, offset 0.5: every position is a cell centre; the last index of each axis takes the upper rule
            for ax, size in zip("xyzt", td):
                n = int(np.prod(td))
                assert c["interp_upper_" + ax] == n // size and c["interp_centre_" + ax] == n - n // size and c["interp_lower_" + ax] == 0
        if name == "two_cells":     # a 2-cell axis: the base index is 0 whichever rule applies
            assert sd[0] == 2 and sd[2] == 2
        for k, v in c.items():
            cnt[k] = cnt.get(k, 0) + v
    for ax in "xyzt":               # both clamp rules and an exact centre on every axis
        for b in ("lower", "upper", "centre"):
            assert cnt["interp_%s_%s" % (b, ax)] > 0, (b, ax)


def test_clamp_rules_of_the_interpolation():
    """the lower rule looks at the position (p < 0, also where truncation already gave index 0), the upper one at the index"""
    data = np.arange(16, dtype=f32).reshape(2, 2, 2, 2)
    one = lambda x: float(M.interpol4d(data, [np.array([v], f32) for v in (x, 0.5, 0.5, 0.5)])[0])
    assert one(0.5) == 0.0 and one(1.0) == 0.5 and one(1.5) == 1.0
    assert one(0.25) == 0.0 and one(-7.0) == 0.0            # p < 0: cell 0 with weights (1, 0)
    assert one(1.75) == 1.0 and one(40.0) == 1.0            # index >= size - 1: cell size - 2 with weights (0, 1)


def test_grid_factor_defaults_and_arguments():
    fac, off = M.grid_factor((4, 4, 4, 4), (8, 8, 8, 8))
    assert np.array_equal(fac, np.full(4, 0.5, f32)) and np.array_equal(off, np.full(4, 0.25, f32))
    fac, off = M.grid_factor((7, 5, 4, 3), (9, 11, 5, 7), offset=(1, 0, 0, 0), scale=(2, 1, 1, 1), size=(14, -1, 0, 7.5))
    assert fac[0] == f32(f32(7) / f32(14)) / f32(2) and off[0] == -f32(1) * fac[0] + fac[0] * f32(0.5)
    assert fac[1] == f32(5) / f32(11) and fac[2] == f32(4) / f32(5)            # size <= 0 keeps the target's size
    assert fac[3] == f32(3) / f32(7.5)


def test_reductions_of_the_vector_types_are_norms():
    a = np.zeros(M.shape_of((2, 2, 2, 2), "vec4"), f32)
    a[1, 0, 1, 0] = (3, 0, 4, 0)
    assert M.reduction("vec4", "getMax", a) == 5 and M.reduction("vec4", "getMaxAbs", a) == 5 and M.reduction("vec4", "getMin", a) == 0
    b = np.full(M.shape_of((2, 2, 2, 2)), -3, f32)
    b[0, 0, 0, 1] = 2
    assert M.reduction("real", "getMaxAbs", b) == 3 and M.reduction("real", "getMax", b) == 2
    assert M.reduction("vec4", "maxDiff", a, np.zeros_like(a)) == 7


def test_recorded_messages():
    want = {
        "save_noext": "file 'noext' does not have an extension", "load_noext": "file 'noext' does not have an extension",
        "save_unknown": "file 'g.foo' filetype not supported", "load_unknown": "file 'g.foo' filetype not supported",
        "construct_2d": "To use 4d grids create a 3d solver with fourthDim>0",
    }
    for k, v in want.items():
        assert str(GOLDEN["message/" + k]) == v
    assert str(GOLDEN["message/construct_no4"]) == str(GOLDEN["message/construct_zero"]) == want["construct_2d"]


# ---- particle data -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", M.PD_KINDS)
def test_pdata_methods_equal_the_reference(kind):
    n_cases = 0
    for key, n, k, op in M.pd_cases():
        if k != kind:
            continue
        a, b, t = M.pd_inputs(key, n, kind, op)
        if op in M.PD_ARRAY_OPS:
            got = M.pd_array_op(kind, op, a, b, t)
        elif op in M.PD_MINMAX:
            got = np.array([M.pd_min_max(kind, op, a)], f32)
        else:
            got = M.pd_sum_reference(M.pd_terms(kind, op, a, t))      # the model of the REFERENCE: one thread, slot order
        msg = M.same_as_fixture(GOLDEN, key, got)
        assert msg is None, msg
        n_cases += 1
    assert n_cases == len(M.PD_SIZES) * (len(M.PD_ARRAY_OPS) + len(M.PD_MINMAX) + 2 * len(M.PD_SUMS))


def test_pdata_masks_and_ranges_do_what_the_cases_exist_for():
    for n in (64, 5000):
        assert (M.pd_flags(n, "all") & M.PD_FLAG).all() and not (M.pd_flags(n, "none") & M.PD_FLAG).any()
        alt = M.pd_flags(n, "alternating") & M.PD_FLAG
        assert alt[::2].all() and not alt[1::2].any()
        s, e = M.pd_range(n)
        assert 0 < s < e < n
        assert (M.pd_rand(n, "real", "b") == 0).any() and (M.pd_rand(n, "int", "b") == 0).any()        # safeDiv meets zeros
    a = np.array([-3, 0.5, 2], f32)
    assert np.array_equal(M.pd_array_op("real", "clampMin", a, a), np.array([-0.6, 0.5, 2], f32))
    assert np.array_equal(M.pd_array_op("real", "clampMax", a, a), np.array([-3, 0.5, 0.9], f32))
    v = np.array([[-3, 0.5, 2]], f32)                                                                  # Vec3: per component
    assert np.array_equal(M.pd_array_op("vec3", "clampMin", v, v), np.array([[-0.6, 0.5, 2]], f32))
    assert np.array_equal(M.pd_array_op("int", "safeDiv", np.array([7, -7, 5], np.int32), np.array([2, 2, 0], np.int32)), np.array([3, -3, 5], np.int32))
    assert np.array_equal(M.pd_norm3(np.array([[0, 0, 0], [1e-7, 0, 0], [1, 0, 0], [3, 4, 0]], f32)), np.array([0, 0, 1, 5], f32))


@pytest.mark.parametrize("kind", M.PD_KINDS)
def test_the_sum_bound_holds_for_the_reference_itself(kind):
    """the bound the device sums are held to is met by the recorded one-thread fp32 sums on the random inputs, and the exactly
    summable inputs are summed exactly"""
    worst = 0.0
    for key, n, k, op in M.pd_cases():
        if k != kind or op not in M.PD_SUMS:
            continue
        a, b, t = M.pd_inputs(key, n, kind, op)
        terms = M.pd_terms(kind, op, a, t)
        ref = GOLDEN[key]
        if terms.dtype == np.int32:
            assert ref.dtype == np.int32 and int(ref[0]) == int(terms.astype(np.int64).sum())          # no wrap at these sizes: exact
            continue
        exact, bound = M.pd_sum_bound(terms)
        err = np.abs(ref.astype(np.float64) - exact)
        assert (err <= bound).all(), (key, err, bound)
        if key.startswith("pdx/"):
            assert (err == 0).all(), key
        elif n > 1:
            worst = max(worst, float((err / np.where(bound > 0, bound, 1)).max()))
    print("%s: the reference's largest error as a share of the bound: %.4f" % (kind, worst))
    assert worst < 1.0


# ---- the harness helpers: checkSymmetry*, testInitGridWithPos, addTestParts ----------------------------------------------------------
def test_symmetry_model_equals_the_reference():
    D = M.sym_digests(GOLDEN)
    cnt, n = {}, 0
    for shape, axis, sym, bound in M.SYM_CASES:
        dims = M.SYM_SHAPES[shape]
        for vec in (False, True):
            for dis in (M.SYM_DISABLE if vec else (0,)):
                for with_err in (True, False):
                    a, err = M.check_symmetry(dims, M.sym_input(shape, vec), with_err, sym, axis, bound, dis, cnt=cnt)
                    key = M.sym_key(shape, axis, sym, bound, vec, dis, with_err)
                    assert M.sha(a) == D[key], key
                    if with_err:
                        assert M.sha(err) == D[key + "/err"], key
                    n += 1
    assert n * 3 // 2 == len(D)
    assert all(cnt[k] > 0 for k in ("sym_pass0", "sym_pass1", "sym_centre", "sym_skipped")), cnt


def test_symmetry_two_passes_are_the_serial_loop_on_1000_random_grids():
    """the restatement the kernels run against the literal FOR_IJK sweep, in which later cells see what earlier cells wrote: even and
    odd sizes, 2-D and 3-D, each axis, both forms, with and without symmetrize / bound / disabled sweeps"""
    r = np.random.default_rng(20240517)
    seen = set()
    for q in range(1000):
        two_d = bool(r.integers(0, 2))
        dims = (int(r.integers(2, 8)), int(r.integers(2, 8)), 1 if two_d else int(r.integers(2, 6)))
        axis = int(r.integers(0, 2 if two_d else 3))
        vec, sym, bound = bool(r.integers(0, 2)), bool(r.integers(0, 2)), int(r.integers(0, 3))
        dis = int(r.integers(0, 8)) if vec else 0
        a = r.uniform(-2, 2, (dims[2], dims[1], dims[0]) + ((3,) if vec else ())).astype(f32)
        if r.integers(0, 4) == 0:                    # an already symmetric input now and then
            a = M.check_symmetry(dims, a, False, True, axis, 0, 0, literal=True)[0]
        la, le = M.check_symmetry(dims, a, True, sym, axis, bound, dis, literal=True)
        ta, te = M.check_symmetry(dims, a, True, sym, axis, bound, dis)
        assert la.tobytes() == ta.tobytes() and le.tobytes() == te.tobytes(), (q, dims, axis, vec, sym, bound, dis)
        seen.add((dims[axis] % 2, axis, vec, sym))
    assert len(seen) == 2 * 3 * 2 * 2                # every combination of parity, axis, form and symmetrize came up


def test_symmetry_properties():
    dims = (6, 4, 1)
    a = M.sym_input("e2", False)[:, :4, :6].copy()
    s, err = M.check_symmetry(dims, a, True, True, 0, 0)
    assert np.array_equal(s[..., :3], s[..., ::-1][..., :3]) and np.array_equal(s[..., 3:], a[..., 3:])      # lower half takes the upper
    assert (err[..., 3:] == 0).all() and (err[..., :3] == np.abs(a[..., :3] - a[..., ::-1][..., :3])).all()  # upper cells see the new lower half
    v = np.zeros((1, 4, 6, 3), f32)
    v[0, 1, 3, 0] = 2                                # MAC, even size: face 3 is the centre line of the normal component
    s, err = M.check_symmetry(dims, v, True, True, 0, 0)
    assert err[0, 1, 3] == 2 and s[0, 1, 3, 0] == 0


def test_init_grid_with_pos_and_add_test_parts_equal_the_reference():
    for shape, dims in M.SYM_SHAPES.items():
        msg = M.same_as_fixture(GOLDEN, "initpos/" + shape, M.init_grid_with_pos(dims))
        assert msg is None, msg
    g = M.init_grid_with_pos((7, 5, 3))
    assert g[0, 0, 0] == 0 and g[0, 0, 1] == 1 and g[0, 4, 3] == 5 and g[2, 0, 0] == 2
    for case in M.ADDPARTS:
        I = M.addparts_inputs(case)
        want = M.add_test_parts(I)
        for k, v in want.items():
            msg = M.same_as_fixture(GOLDEN, "addparts/%s/%s" % (case, k), v)
            assert msg is None, msg
        assert len(want["pos"]) == I["n0"] + I["num"]
    assert (M.addparts_inputs("populated")["flags"] & M.PNEW).any()           # PNEW is set on some old slots, and must be cleared
