"""CPU: the numpy statement of the array bridge and the MLFLIP data plugins (tests/mlflip_model.py) against the reference's recorded
outputs (tests/golden/mlflip.npz, recorded by tools/record_mlflip.py), bit for bit; and the order-free statement of the region
labelling against the reference's serial flood fill as written, on 1000 random small grids."""
import os

import numpy as np
import pytest

import mlflip_model as M

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlflip.npz")
GOLDEN = np.load(GOLDEN_PATH)
f32, f64, i32 = np.float32, np.float64, np.int32
DTYPES = {"i": i32, "f": f32, "d": f64}
KINDS = {"real": "real", "flag": "int", "levelset": "real", "vec3": "vec", "mac": "vec"}


def test_the_fixture_is_small_and_complete():
    assert os.path.getsize(GOLDEN_PATH) < 1000000
    keys = set(GOLDEN.files)
    for name in M.REGION_CASES:
        for k in ("r", "count", "rcnt", "ext", "marked"):
            assert "region/%s/%s" % (name, k) in keys
    for name in M.FEATURE_CASES:
        assert "feat/%s" % name in keys or "feat/%s#sha" % name in keys
    for kind in KINDS:
        for d in DTYPES:
            if KINDS[kind] == "vec" and d == "i":
                continue
            assert "copy/to_grid/%s/%s" % (kind, d) in keys and "copy/to_array/%s/%s" % (kind, d) in keys


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_copies_convert_as_the_reference_does(kind):
    A = M.copy_inputs()
    mk = KINDS[kind]
    for d, dt in DTYPES.items():
        if mk == "vec" and d == "i":
            continue
        src = A["v" + d] if mk == "vec" else A[d]
        assert M.same_as_fixture(GOLDEN, "copy/to_grid/%s/%s" % (kind, d), M.array_to_grid(src, M.COPY_DIMS, mk)) is None
        grid = M.array_to_grid(A["vf"] if mk == "vec" else (A["i"] if mk == "int" else A["f"]), M.COPY_DIMS, mk)
        assert M.same_as_fixture(GOLDEN, "copy/to_array/%s/%s" % (kind, d), M.grid_to_array(grid, dt)) is None


def test_the_copy_inputs_separate_the_conversions():
    A = M.copy_inputs()
    g = GOLDEN["copy/to_grid/real/i"].reshape(-1)
    assert A["i"].reshape(-1)[0] == 2 ** 24 + 1 and g[0] == f32(2 ** 24)                      # int -> float rounds to nearest even
    assert A["i"].reshape(-1)[2] == 2 ** 24 + 3 and g[2] == f32(2 ** 24 + 4)
    g = GOLDEN["copy/to_grid/real/d"].reshape(-1)
    assert A["d"].reshape(-1)[0] == 1 + 2.0 ** -30 and g[0] == f32(1)                        # double -> float rounds
    assert g[5] == np.nextafter(f32(1), f32(2))                                              # 1 + 2^-24 + 2^-40: above the tie, up
    g = GOLDEN["copy/to_grid/flag/d"].reshape(-1)
    assert g[1] == -1 and g[2] == 1 and g[3] == 0 and g[4] == 2                              # -1.7, 1.7, -0.999, 2.5 towards zero
    assert GOLDEN["copy/to_array/real/i"].reshape(-1)[1] == -1


def test_pdata_copy_and_simple_numpy_test():
    A = M.copy_inputs()
    assert M.same_as_fixture(GOLDEN, "copy/pdata_vec3", np.ascontiguousarray(A["vf"].reshape(-1, 3))) is None
    sx, sy, sz = M.COPY_DIMS
    arr = np.ascontiguousarray(A["d"].astype(f32).reshape(-1)[:sx * sy + 5])
    assert M.same_as_fixture(GOLDEN, "simple", M.simple_numpy_test(A["f"], arr, 0.375)) is None


@pytest.mark.parametrize("name", sorted(M.FEATURE_CASES))
def test_features_match_the_reference(name):
    I = M.feature_inputs(name)
    for w in range(I["window"] + 1):
        assert M.geo_precondition(I["dims"], I["pos"], w)
    fv = M.feature_matrix(I)
    assert M.same_as_fixture(GOLDEN, "feat/%s" % name, fv) is None
    live = (I["pflag"] & M.PDELETE) == 0
    if I["ptype"] is not None:
        live &= (I["ptype"] & I["exclude"]) == 0
    assert live.any() and (I["ptype"] is None or not live.all())
    assert (fv[~live] == M.FILL).all()                                                      # skipped rows are not written
    used = I["off_begin"] + sum(I["widths"])
    assert (fv[:, :I["off_begin"]] == M.FILL).all() and (fv[:, used:] == M.FILL).all()       # nor the rest of a row
    assert not (fv[live][:, I["off_begin"]:used] == M.FILL).any()


def test_stencil_order():
    assert M.stencil(1, True)[:4].tolist() == [[-1, -1, -1], [-1, -1, 0], [-1, -1, 1], [-1, 0, -1]]
    assert M.stencil(1, False).tolist() == [[i, j, 0] for i in (-1, 0, 1) for j in (-1, 0, 1)]
    assert len(M.stencil(2, True)) == 125 and M.stencil(0, True).tolist() == [[0, 0, 0]]
    assert M.feature_width("vel", 1, True) == 81 and M.feature_width("vel", 1, False) == 18 and M.feature_width("geo", 2, False) == 25


@pytest.mark.parametrize("name", sorted(M.REGION_CASES))
def test_regions_match_the_reference(name):
    flags = M.region_flags(name)
    assert M.border_free(flags, M.FLUID)
    r, count = M.regions(flags, M.FLUID)
    assert count == int(GOLDEN["region/%s/count" % name][0])
    rcnt = M.regional_counts(flags, M.FLUID)
    for key, got in (("r", r), ("rcnt", rcnt), ("ext", M.extend_region(flags, **M.REGION_EXTEND)),
                     ("marked", M.mark_small_regions(flags, rcnt, **M.REGION_MARK))):
        assert np.array_equal(got, GOLDEN["region/%s/%s" % (name, key)].astype(i32)), key
    assert rcnt.max() < 20000                       # the reference recurses once per cell


def test_order_free_labelling_equals_the_serial_flood_fill():
    rng = np.random.RandomState(20240607)
    seen = 0
    for case in range(1000):
        if case % 2:
            dims = (int(rng.randint(3, 10)), int(rng.randint(3, 9)), 1)
        else:
            dims = (int(rng.randint(3, 8)), int(rng.randint(3, 7)), int(rng.randint(3, 6)))
        sx, sy, sz = dims
        vals = np.array([1, 2, 4, 1 | 64, 4 | 16], i32)
        flags = rng.choice(vals, size=(sz, sy, sx), p=[0.35, 0.1, 0.25, 0.2, 0.1]).astype(i32)
        ctype = [1, 4, 1 | 4, 64][case % 4]
        border = ~M.clear_border(np.ones(flags.shape, bool))
        flags[border] = 2
        assert M.border_free(flags, ctype)
        r, count = M.regions(flags, ctype)
        fr, fcount = M.flood_fill_regions(flags, ctype)
        assert count == fcount and np.array_equal(r, fr), (case, dims)
        rc = M.regional_counts(flags, ctype)
        want = np.where(fr > 0, np.bincount(fr.reshape(-1), minlength=fcount + 1)[fr], 0)
        assert np.array_equal(rc, want), (case, dims)
        seen += count > 1
    assert seen >= 250                              # the inputs: at least a quarter of the cases has several regions to number


@pytest.mark.parametrize("dims", [(7, 5, 4), (12, 9, 1)])
def test_extend_region_is_two_phase_and_stops_at_the_grid(dims):
    """literal restatement of tfplugins.cpp:190-207 (collect, then assign) against the model's array form"""
    sx, sy, sz = dims
    rng = np.random.RandomState(5)
    flags = rng.choice(np.array([1, 2, 4, 1 | 64, 4 | 16, 2 | 4], i32), size=(sz, sy, sx)).astype(i32)
    region, exclude = 4, 2
    for depth in (0, 1, 3, 50):
        f = flags.copy()
        for _ in range(depth):
            upd = []
            for k in range(sz):
                for j in range(sy):
                    for i in range(sx):
                        if f[k, j, i] & exclude:
                            continue
                        if ((i > 0 and f[k, j, i - 1] & region) or (i < sx - 1 and f[k, j, i + 1] & region) or (j > 0 and f[k, j - 1, i] & region)
                                or (j < sy - 1 and f[k, j + 1, i] & region)
                                or (sz > 1 and ((k > 0 and f[k - 1, j, i] & region) or (k < sz - 1 and f[k + 1, j, i] & region)))):
                            upd.append((k, j, i))
            for c in upd:
                f[c] = region
        assert np.array_equal(M.extend_region(flags, region, exclude, depth), f), depth
