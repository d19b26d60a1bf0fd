"""GPU: the array bridge and the MLFLIP data plugins (include/open/manta_hip_mlflip.h) against the numpy statement of
tests/mlflip_model.py and the reference's recorded outputs (tests/golden/mlflip.npz), bit for bit throughout.  Outputs are pre-filled with
NaN or garbage; arrays go in and out as numpy arrays, CPU tensors and tensors on the solver's device."""
import os

import numpy as np
import pytest
import torch

import mlflip_model as M

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlflip.npz"))
f32, f64, i32 = np.float32, np.float64, np.int32
DTYPES = {"i": i32, "f": f32, "d": f64}
KINDS = {"Real": "real", "Flag": "int", "Levelset": "real", "Vec3": "vec", "MAC": "vec"}      # plugin suffix -> the model's kind
FORMS = ("numpy", "cpu", "device")
GARBAGE = -12345


def solver(m, dims):
    return m.Solver(name="s", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)


def as_form(a, form, s):
    """a copy of the numpy array as a numpy array, a CPU tensor or a tensor on the solver's device"""
    if form == "numpy":
        return a.copy()
    t = torch.from_numpy(a.copy())
    return t if form == "cpu" else t.to(s.device)


def back(t, s):
    if isinstance(t, np.ndarray):
        return t
    s.sync()
    return t.cpu().numpy()


def poison(g):
    if g.data.dtype == torch.int32:
        g.data.fill_(GARBAGE)
    else:
        g.data.fill_(float("nan"))


def grid_of(m, s, kind):
    return s.create({"Real": m.RealGrid, "Flag": m.FlagGrid, "Levelset": m.LevelsetGrid, "Vec3": m.VecGrid, "MAC": m.MACGrid}[kind])


def junk(shape, dt):
    return np.full(shape, np.nan if dt != i32 else GARBAGE, dt)


def bits(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, got.dtype, want.shape, want.dtype)
    u = "u%d" % got.dtype.itemsize
    d = np.argwhere(got.view(u) != want.view(u))
    assert len(d) == 0, "%s: %d of %d words differ, first at %s: %r, expected %r" % (tag, len(d), got.size, d[0], got[tuple(d[0])], want[tuple(d[0])])


# ---- grid copies ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(7, 5, 4), (33, 31, 29), (12, 9, 1), (3, 3, 1)])
def test_grid_copies_every_kind_type_and_form(hip_backend, dims):
    import manta as m
    s = solver(m, dims)
    sx, sy, sz = dims
    A = M.copy_inputs(dims)
    for kind, mk in KINDS.items():
        to_grid, to_array = getattr(m, "copyArrayToGrid" + kind), getattr(m, "copyGridToArray" + kind)
        g = grid_of(m, s, kind)
        for d, dt in DTYPES.items():
            if mk == "vec" and d == "i":
                continue
            src = A["v" + d] if mk == "vec" else A[d]
            want = M.array_to_grid(src, dims, mk)
            for form in FORMS:
                tag = "%s %s %s" % (kind, d, form)
                poison(g)
                to_grid(as_form(src, form, s), g)
                bits("to grid " + tag, g.to_numpy(), want)
                t = as_form(junk(src.shape, dt), form, s)
                ptr = t.data_ptr() if form != "numpy" else t.ctypes.data
                to_array(g, t)
                assert (t.data_ptr() if form != "numpy" else t.ctypes.data) == ptr
                bits("to array " + tag, back(t, s), M.grid_to_array(want, dt))
                if dims == M.COPY_DIMS:
                    assert M.same_as_fixture(GOLDEN, "copy/to_grid/%s/%s" % (kind.lower(), d), want) is None
            # the [z][y][x][1] shape of a scalar array, and a source that is not C-contiguous
            if mk != "vec":
                poison(g)
                to_grid(as_form(src.reshape(sz, sy, sx, 1), "device", s), g)
                bits("4-D " + kind + d, g.to_numpy(), want)
                t = junk((sz, sy, sx, 1), dt)
                to_array(g, t)
                bits("4-D back " + kind + d, t.reshape(sz, sy, sx), M.grid_to_array(want, dt))
            fortran = np.asfortranarray(src)
            if src.size > 1 and sx > 1:
                assert not fortran.flags["C_CONTIGUOUS"]
            for form in FORMS:
                t = fortran.copy(order="F") if form == "numpy" else torch.from_numpy(fortran.copy(order="F"))
                if form == "device":
                    t = t.to(s.device)
                    assert not t.is_contiguous() or src.size == 1
                poison(g)
                to_grid(t, g)
                bits("strided source " + kind + d + form, g.to_numpy(), want)


def test_round_trips_and_the_fixture(hip_backend):
    import manta as m
    dims = M.COPY_DIMS
    s = solver(m, dims)
    A = M.copy_inputs(dims)
    for kind, mk in KINDS.items():
        g, g2 = grid_of(m, s, kind), grid_of(m, s, kind)
        for d, dt in DTYPES.items():
            if mk == "vec" and d == "i":
                continue
            src = A["v" + d] if mk == "vec" else A[d]
            poison(g)
            getattr(m, "copyArrayToGrid" + kind)(src, g)
            assert M.same_as_fixture(GOLDEN, "copy/to_grid/%s/%s" % (kind.lower(), d), g.to_numpy()) is None
            # the grid the recorder used for the way back
            g.from_numpy(M.array_to_grid(A["vf"] if mk == "vec" else (A["i"] if mk == "int" else A["f"]), dims, mk))
            arr = junk(g.to_numpy().shape, dt)
            getattr(m, "copyGridToArray" + kind)(g, arr)
            assert M.same_as_fixture(GOLDEN, "copy/to_array/%s/%s" % (kind.lower(), d), arr) is None
            # array -> grid -> array -> grid: the second grid is the first
            if not (mk == "int" and d != "i") and not (mk != "int" and d == "i"):
                poison(g2)
                getattr(m, "copyArrayToGrid" + kind)(arr, g2)
                bits("round trip " + kind + d, g2.to_numpy(), g.to_numpy())


def test_simple_numpy_test(hip_backend):
    import manta as m
    sx, sy, sz = M.COPY_DIMS
    s = solver(m, M.COPY_DIMS)
    A = M.copy_inputs()
    arr = np.ascontiguousarray(A["d"].astype(f32).reshape(-1)[:sx * sy + 5])
    for form in FORMS:
        g = s.create(m.RealGrid)
        g.from_numpy(A["f"])
        m.simpleNumpyTest(g, as_form(arr, form, s), 0.375)
        assert M.same_as_fixture(GOLDEN, "simple", g.to_numpy()) is None, form
    s2 = solver(m, (12, 9, 1))
    g = s2.create(m.RealGrid)
    base = np.random.RandomState(2).rand(1, 9, 12).astype(f32)
    g.from_numpy(base)
    arr = np.random.RandomState(3).rand(12 * 9).astype(f32)
    m.simpleNumpyTest(g, arr, -1.25)
    bits("2-D", g.to_numpy(), M.simple_numpy_test(base, arr, -1.25))


# ---- particle data copies ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 100003])
def test_pdata_copies(hip_backend, n):
    import manta as m
    s = solver(m, (8, 8, 8))
    pp = s.create(m.BasicParticleSystem)
    pI, pR, pV = pp.create(m.PdataInt), pp.create(m.PdataReal), pp.create(m.PdataVec3)
    pp.set_positions(np.zeros((n, 3), f32))
    pp.reserve(n + 37)
    cap = pp.cap
    assert cap >= n + 37 and pI.cap == cap and pV.cap == cap and pI.size() == n
    rng = np.random.RandomState(n + 1)
    src = {"Int": rng.randint(-2 ** 31, 2 ** 31 - 1, n).astype(i32), "Real": rng.rand(n).astype(f32), "Vec3": rng.rand(n, 3).astype(f32)}
    src["Real"][:1] = np.nan
    for kind, pd in (("Int", pI), ("Real", pR), ("Vec3", pV)):
        a = src[kind]
        dt = a.dtype.type
        for form in FORMS:
            for shape in ((a.shape, (3 * n,)) if kind == "Vec3" else (a.shape,)):
                pd.data.fill_(GARBAGE if kind == "Int" else float("nan"))
                getattr(m, "copyArrayToPdata" + kind)(as_form(a.reshape(shape), form, s), pd)
                s.sync()
                planes = pd.data.cpu().numpy().reshape(pd._ncomp, cap)
                bits("to pdata %s %s" % (kind, form), planes[:, :n], np.ascontiguousarray(a.reshape(n, pd._ncomp).T))
                tail = planes[:, n:]
                assert (tail == GARBAGE).all() if kind == "Int" else np.isnan(tail).all()       # the slots past size() are not touched
                t = as_form(junk(shape, dt), form, s)
                ptr = t.data_ptr() if form != "numpy" else t.ctypes.data
                getattr(m, "copyPdataToArray" + kind)(pd, t)
                assert (t.data_ptr() if form != "numpy" else t.ctypes.data) == ptr
                bits("to array %s %s" % (kind, form), back(t, s).reshape(a.shape), a)
        if kind == "Vec3" and n > 1:                        # a strided source
            wide = np.zeros((n, 6), f32)
            wide[:, ::2] = a
            pd.data.fill_(float("nan"))
            m.copyArrayToPdataVec3(wide[:, ::2], pd)
            bits("strided", pd.to_numpy(), a)


# ---- features ---------------------------------------------------------------------------------------------------------------------
def pkg_extract(m, s, grids, pp, pT, form):
    """the model's `extract` callable on the package: one plugin call on a matrix in the given form"""
    def extract(kind, dims, grid, pos, pflag, ptype, exclude, window, scale, fv, N_row, off_begin):
        t = as_form(np.ascontiguousarray(fv, f32), form, s)
        plug = {"vel": m.extractFeatureVel, "phi": m.extractFeaturePhi, "geo": m.extractFeatureGeo}[kind]
        plug(t, N_row, off_begin, pp, grids[kind], scale, pT if ptype is not None else None, exclude, window)
        return back(t, s).reshape(np.shape(fv))
    return extract


def stage_features(m, I):
    s = solver(m, I["dims"])
    vel, phi, flags = s.create(m.MACGrid), s.create(m.LevelsetGrid), s.create(m.FlagGrid)
    vel.from_numpy(I["vel"]); phi.from_numpy(I["phi"]); flags.from_numpy(I["flags"])
    pp = s.create(m.BasicParticleSystem)
    pT = pp.create(m.PdataInt)
    pp.set_positions(I["pos"], I["pflag"])
    pp.reserve(I["n"] + 11)                                  # a capacity larger than the size
    if I["n"]:
        pT.from_numpy(I["ptype"] if I["ptype"] is not None else np.zeros(I["n"], i32))
    return s, dict(vel=vel, phi=phi, geo=flags), pp, pT


@pytest.mark.parametrize("name", sorted(M.FEATURE_CASES))
def test_features_fixture_cases(hip_backend, name):
    import manta as m
    I = M.feature_inputs(name)
    assert M.geo_precondition(I["dims"], I["pos"], I["window"])
    s, grids, pp, pT = stage_features(m, I)
    got = {form: M.feature_matrix(I, pkg_extract(m, s, grids, pp, pT, form)) for form in FORMS}
    for form in FORMS:
        assert M.same_as_fixture(GOLDEN, "feat/%s" % name, got[form]) is None, form
    assert got["numpy"].tobytes() == got["device"].tobytes() == got["cpu"].tobytes()


def seeded_features(dims, n, window, use_ptype, seed):
    vel, phi, flags = M.smooth_fields(dims, seed)
    pos, pflag, ptype = M.feature_particles(dims, n, window, seed + 1)
    is3d = dims[2] > 1
    widths = [M.feature_width(k, window, is3d) for k in ("vel", "phi", "geo")]
    return dict(dims=dims, vel=vel, phi=phi, flags=flags, pos=pos, pflag=pflag, ptype=ptype if use_ptype else None, exclude=2, window=window,
                scale=0.625, off_begin=3, widths=widths, N_row=3 + sum(widths) + 6, n=n)


@pytest.mark.parametrize("dims", [(33, 31, 29), (37, 29, 1)])
@pytest.mark.parametrize("window,n,use_ptype", [(0, 10007, True), (1, 10007, True), (2, 1501, True), (1, 1, True), (1, 0, True), (1, 257, False)])
def test_features_equal_the_model_on_seeded_inputs(hip_backend, dims, window, n, use_ptype):
    import manta as m
    I = seeded_features(dims, n, window, use_ptype, 3 * window + n % 7)
    assert M.geo_precondition(dims, I["pos"], window)
    if n > 100:
        live = (I["pflag"] & M.PDELETE) == 0
        assert not live.all() and live.any()
    want = M.feature_matrix(I)
    s, grids, pp, pT = stage_features(m, I)
    got = M.feature_matrix(I, pkg_extract(m, s, grids, pp, pT, "numpy"))
    bits("numpy target", got, want)
    dev = M.feature_matrix(I, pkg_extract(m, s, grids, pp, pT, "device"))
    assert dev.tobytes() == got.tobytes()


def test_features_write_a_device_tensor_in_place(hip_backend):
    """a model on the same device reads the matrix where the kernel wrote it: same storage, no host copy, stream order only"""
    import manta as m
    I = seeded_features((33, 31, 29), 4099, 1, True, 9)
    s, grids, pp, pT = stage_features(m, I)
    fv = torch.full((I["n"], I["N_row"]), float(M.FILL), dtype=torch.float32, device=s.device)
    ptr, off = fv.data_ptr(), I["off_begin"]
    m.extractFeatureVel(fv, I["N_row"], off, pp, grids["vel"], I["scale"], pT, I["exclude"], 1)
    m.extractFeaturePhi(fv, I["N_row"], off + I["widths"][0], pp, grids["phi"], I["scale"], pT, I["exclude"], 1)
    m.extractFeatureGeo(fv, I["N_row"], off + I["widths"][0] + I["widths"][1], pp, grids["geo"], I["scale"], pT, I["exclude"], 1)
    total = fv.sum(dim=1)                       # a consumer on the same stream, before any synchronisation
    s.sync()
    assert fv.data_ptr() == ptr
    want = M.feature_matrix(I)
    bits("in place", fv.cpu().numpy(), want)
    assert np.allclose(total.cpu().numpy(), want.astype(f64).sum(1), rtol=1e-4)
    # a contiguous view into a larger tensor is written where it is, the rest stays
    big = torch.full((I["n"] + 4, I["N_row"]), 3.0, dtype=torch.float32, device=s.device)
    view = big[2:I["n"] + 2]
    view.fill_(float(M.FILL))
    m.extractFeaturePhi(view, I["N_row"], off + I["widths"][0], pp, grids["phi"], I["scale"], pT, I["exclude"], 1)
    s.sync()
    only_phi = M.extract_feature("phi", I["dims"], I["phi"], I["pos"], I["pflag"], I["ptype"], I["exclude"], 1, I["scale"],
                                 np.full((I["n"], I["N_row"]), M.FILL, f32), I["N_row"], off + I["widths"][0])
    bits("view", big[2:I["n"] + 2].cpu().numpy(), only_phi)
    assert (big[:2] == 3.0).all().item() and (big[I["n"] + 2:] == 3.0).all().item()


# ---- regions ----------------------------------------------------------------------------------------------------------------------
def run_regions(m, s, flags_np, ctype):
    """getRegions and getRegionalCounts, each twice into poisoned grids -> (r, count, rcnt)"""
    flags = s.create(m.FlagGrid)
    flags.from_numpy(flags_np)
    outs = []
    for rep in range(2):
        r, rc = s.create(m.IntGrid), s.create(m.IntGrid)
        r.data.fill_(GARBAGE - rep)
        rc.data.fill_(GARBAGE - rep)
        # the pool's scratch is garbage as well
        scratch = [s.create(m.IntGrid) for _ in range(2)]
        for g in scratch:
            g.data.fill_(0x7fffffff - rep)
        del scratch
        count = m.getRegions(r, flags, ctype)
        m.getRegionalCounts(rc, flags, ctype)
        outs.append((r.to_numpy(), count, rc.to_numpy()))
    bits("flags are read only", flags.to_numpy(), flags_np)
    assert outs[0][1] == outs[1][1] and outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][2].tobytes() == outs[1][2].tobytes()
    return outs[0]


@pytest.mark.parametrize("name", sorted(M.REGION_CASES))
def test_regions_fixture_cases(hip_backend, name):
    import manta as m
    flags_np = M.region_flags(name)
    assert M.border_free(flags_np, M.FLUID)
    dims = M.REGION_CASES[name][0]
    s = solver(m, dims)
    r, count, rc = run_regions(m, s, flags_np, M.FLUID)
    assert count == int(GOLDEN["region/%s/count" % name][0])
    bits("r", r, GOLDEN["region/%s/r" % name].astype(i32))
    bits("rcnt", rc, GOLDEN["region/%s/rcnt" % name].astype(i32))
    flags, rcg = s.create(m.FlagGrid), s.create(m.IntGrid)
    flags.from_numpy(flags_np)
    m.extendRegion(flags, **M.REGION_EXTEND)
    bits("ext", flags.to_numpy(), GOLDEN["region/%s/ext" % name].astype(i32))
    flags.from_numpy(flags_np)
    rcg.from_numpy(rc)
    m.markSmallRegions(flags, rcg, **M.REGION_MARK)
    bits("marked", flags.to_numpy(), GOLDEN["region/%s/marked" % name].astype(i32))


@pytest.mark.parametrize("dims", [(7, 5, 4), (33, 31, 29), (12, 9, 1), (40, 37, 1), (3, 3, 1), (130, 5, 4), (67, 59, 53)])
def test_region_patterns_equal_the_model(hip_backend, dims):
    """(130, 5, 4): rows of three 64-cell segments, so runs cross the seam between two wavefronts; (67, 59, 53): about 200 000 cells,
    so the numbering's scan spans several blocks"""
    import manta as m
    s = solver(m, dims)
    for name in M.REGION_PATTERNS:
        flags_np, ctype = M.region_pattern(name, dims)
        assert M.border_free(flags_np, ctype)
        r, count, rc = run_regions(m, s, flags_np, ctype)
        want, wcount = M.regions(flags_np, ctype)
        assert count == wcount, name
        bits(name + " r", r, want)
        bits(name + " rcnt", rc, M.regional_counts(flags_np, ctype))


@pytest.mark.parametrize("dims", [(7, 5, 4), (12, 9, 1), (33, 31, 29), (3, 3, 1)])
def test_extend_region(hip_backend, dims):
    import manta as m
    sx, sy, sz = dims
    s = solver(m, dims)
    rng = np.random.RandomState(sx)
    base = rng.choice(np.array([1, 2, 1 | 64, 2 | 4, 1 | 256, 8], i32), size=(sz, sy, sx), p=[0.45, 0.2, 0.15, 0.05, 0.1, 0.05]).astype(i32)
    region, exclude = 4, 2
    # region cells on every face of the grid, some carrying other bits
    base[sz // 2, sy // 2, 0] = 4
    base[sz // 2, sy // 2, sx - 1] = 4 | 16
    base[sz // 2, 0, sx // 2] = 4
    base[sz // 2, sy - 1, sx // 2] = 4 | 64
    base[0, sy // 2, sx // 2] = 4
    base[sz - 1, sy // 2, sx // 2] = 4 | 1
    assert ((base & exclude) != 0).any() and ((base & region) != 0).any()
    flags = s.create(m.FlagGrid)
    for depth in (0, 1, 2, 3, sx + sy + sz + 40):
        flags.from_numpy(base)
        tmp = s.create(m.IntGrid)
        tmp.data.fill_(GARBAGE)
        del tmp                                              # the pool grid the plugin ping-pongs with
        m.extendRegion(flags, region, exclude, depth)
        bits("depth %d" % depth, flags.to_numpy(), M.extend_region(base, region, exclude, depth))
    flags.from_numpy(base)
    m.extendRegion(flags, 4 | 1, 2 | 8, 2)                    # masks of two bits
    bits("two bits", flags.to_numpy(), M.extend_region(base, 4 | 1, 2 | 8, 2))


def test_mark_small_regions(hip_backend):
    import manta as m
    dims = (33, 31, 29)
    s = solver(m, dims)
    flags_np = M.region_flags("r33_55")
    rcnt_np = M.regional_counts(flags_np, M.FLUID)
    sizes = np.unique(rcnt_np[rcnt_np > 0])
    assert sizes.size > 3
    size, larger = int(sizes[len(sizes) // 2]), int(sizes[len(sizes) // 2 + 1])      # two sizes that regions of the case have
    assert size > 1
    flags, rcnt = s.create(m.FlagGrid), s.create(m.IntGrid)
    rcnt.from_numpy(rcnt_np)
    seen = set()
    for th in (size - 1, size, larger, 0, 10 ** 6):
        for exclude in (M.OBSTACLE, M.OBSTACLE | M.EMPTY):
            flags.from_numpy(flags_np)
            m.markSmallRegions(flags, rcnt, M.EMPTY | 256, exclude, th)
            want = M.mark_small_regions(flags_np, rcnt_np, M.EMPTY | 256, exclude, th)
            bits("th %d" % th, flags.to_numpy(), want)
            seen.add(want.tobytes())
    assert len(seen) == 10                                   # every threshold and every mask decides some cell differently
    flags.from_numpy(flags_np)
    m.markSmallRegions(flags, rcnt, M.EMPTY, M.OBSTACLE)      # th = 1
    bits("default th", flags.to_numpy(), M.mark_small_regions(flags_np, rcnt_np, M.EMPTY, M.OBSTACLE, 1))


# ---- one loop ---------------------------------------------------------------------------------------------------------------------
def test_data_generation_loop_against_the_recorded_run(hip_backend):
    """flip01_simple.py's 3-D dam break at 32^3 for 8 steps with the per-frame calls of manta_gendata.py beside it"""
    import manta as m
    C = M.LOOP
    counts, snaps = M.gendata_loop(m, "numpy")
    print("loop counts (particles, regions, labelled cells, particles with a label):\n", counts)
    assert np.array_equal(counts, GOLDEN["loop/counts"]), (counts, GOLDEN["loop/counts"])
    for q, step in enumerate(C["snaps"]):
        fv, labels, pvel, pos = snaps[step]
        assert fv.shape[0] == int(GOLDEN["loop/np"][q])
        assert M.geo_precondition((C["res"],) * 3, pos, C["window"])
        rows = fv[::C["every"]]
        bits("labels %d" % step, labels, GOLDEN["loop/labels%d" % step].astype(i32))
        bits("feature head %d" % step, rows[:C["head"]], GOLDEN["loop/fvhead%d" % step])
        assert M.same_as_fixture(GOLDEN, "loop/fv%d" % step, rows) is None
        assert M.same_as_fixture(GOLDEN, "loop/pvel%d" % step, pvel[::C["every"]]) is None
        excluded = (labels & M.FLUID) != 0
        assert excluded.any() and not excluded.all()
        assert (fv[excluded] == M.FILL).all() and not (fv[~excluded] == M.FILL).any()
