"""GPU: the 4-D grids on the device (include/open/manta_hip_grid4d.h and the core entries behind the flat float operators) against the
fixture recorded from the compiled reference (tests/golden/grid4d.npz), bit for bit, for all four element types.  Outputs and pool
storage are pre-filled with NaN / garbage, every call runs after the same call on a larger solver and then twice in a row.  Nothing
here reads the reference tree."""
import os

import numpy as np
import pytest
import torch

import grid4d_model as M

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid4d.npz"))
CLS = {"real": "Grid4Real", "int": "Grid4Int", "vec3": "Grid4Vec3", "vec4": "Grid4Vec4"}
LARGER = (35, 9, 6, 5)


def _solver(m, dims, poison=True):
    s = m.Solver(name="s4", gridSize=m.vec3(*dims[:3]), dim=3, fourthDim=dims[3])
    if poison:                  # what the pool hands out must be zeroed by the pool, not by luck
        n = int(np.prod(dims))
        for kind, nc in M.NCOMP.items():
            for _ in range(3):
                t = torch.full((nc * n,), 0x7f7f7f7f, dtype=torch.int32, device=s.device) if kind == "int" else \
                    torch.full((nc * n,), float("nan"), dtype=torch.float32, device=s.device)
                s._pool4.setdefault(kind, []).append(t)
    return s


def _grid(m, s, kind, arr=None):
    g = s.create(getattr(m, CLS[kind]))
    if arr is not None:
        g.from_numpy(arr)
    return g


def _value(m, kind, v):
    return v if kind in ("real", "int") else (m.vec3(*v) if kind == "vec3" else m.vec4(*v))


def _run_op(m, s, dims, kind, op, arg):
    """one case of M.op_cases() through the package: the array, or the scalar as a float32 array of one"""
    a, b = _grid(m, s, kind, M.rand_grid(dims, kind, "a")), _grid(m, s, kind, M.rand_grid(dims, kind, "b"))
    if op in ("add", "sub", "mult"):
        getattr(a, op)(b)
    elif op in ("setConst", "addConst", "multConst"):
        getattr(a, op)(_value(m, kind, M.CONST[kind]))
    elif op == "addScaled":
        a.addScaled(b, _value(m, kind, M.FACTOR[kind]))
    elif op == "clamp":
        a.clamp(*M.CLAMP[kind])
    elif op in ("getMin", "getMax", "getMaxAbs"):
        r = np.array([getattr(a, op)()], f32)
        assert np.array_equal(a.to_numpy(), M.rand_grid(dims, kind, "a"))
        return r
    elif op == "maxDiff":
        fn = {"real": m.grid4dMaxDiff, "int": m.grid4dMaxDiffInt, "vec3": m.grid4dMaxDiffVec3, "vec4": m.grid4dMaxDiffVec4}[kind]
        return np.array([fn(a, b)], f32)
    elif op == "setBound":
        a.setBound(_value(m, kind, M.CONST[kind]), arg)
    elif op == "setBoundNeumann":
        a.setBoundNeumann(arg)
    else:
        raise KeyError(op)
    assert np.array_equal(b.to_numpy(), M.rand_grid(dims, kind, "b"))
    return a.to_numpy()


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("shape", sorted(M.SHAPES) + sorted(M.NEUMANN))
def test_operators_reductions_and_boundaries(hip_backend, shape, kind):
    import manta as m
    cases = [c for c in M.op_cases() if c[1] == shape and c[3] == kind]
    assert cases
    dims = cases[0][2]
    big, s = _solver(m, LARGER), _solver(m, dims)
    assert not np.any(_grid(m, s, kind).to_numpy())                                  # a poisoned pool hands out zeros
    for key, name, dims, kind, op, arg in cases:
        if op != "setBoundNeumann" or min(LARGER) >= 2 * arg + 3:
            _run_op(m, big, LARGER, kind, op, arg)
        for rep in range(2):
            got = _run_op(m, s, dims, kind, op, arg)
            msg = M.same_as_fixture(GOLDEN, key, got)
            assert msg is None, "%s (run %d)" % (msg, rep)


def test_neumann_below_its_precondition_is_refused(hip_backend):
    import manta as m
    g = _grid(m, _solver(m, (5, 5, 5, 4)), "real", M.rand_grid((5, 5, 5, 4), "real", "a"))
    with pytest.raises(RuntimeError) as err:
        g.setBoundNeumann(1)
    assert "too small for boundaryWidth 1" in str(err.value)
    assert np.array_equal(g.to_numpy(), M.rand_grid((5, 5, 5, 4), "real", "a"))


def test_copy_clear_and_zeroed_storage(hip_backend):
    import manta as m
    dims = M.SHAPES["c"]
    s = _solver(m, dims)
    for kind in M.KINDS:
        A = M.rand_grid(dims, kind, "a")
        a, b = _grid(m, s, kind, A), _grid(m, s, kind, M.garbage(dims, kind))
        assert b.copyFrom(a) is b and np.array_equal(b.to_numpy(), A) and a.to_numpy().tobytes() == A.tobytes()
        a.clear()
        assert not np.any(a.to_numpy())


def test_regions_slices_and_components(hip_backend):
    import manta as m
    dims = M.SHAPES["a"]
    big = _solver(m, LARGER)
    m.setRegion4d(_grid(m, big, "real"), m.vec4(1), m.vec4(3), 2.0)
    s = _solver(m, dims)
    for rep in range(2):
        for rname, (start, end) in M.REGIONS.items():
            for kind in ("real", "vec4"):
                g = _grid(m, s, kind, M.rand_grid(dims, kind, "a"))
                (m.setRegion4d if kind == "real" else m.setRegion4dVec4)(g, m.vec4(*start), m.vec4(*end), _value(m, kind, M.REGION_VALUE[kind]))
                msg = M.same_as_fixture(GOLDEN, "region/%s/%s" % (rname, kind), g.to_numpy())
                assert msg is None, msg
        for sname, (shape, srct, dd) in M.SLICES.items():
            sd = M.SHAPES[shape]
            s4, s3 = _solver(m, sd), m.Solver(name="s3", gridSize=m.vec3(*dd), dim=3)
            dsh = (dd[2], dd[1], dd[0])
            for kind in ("real", "vec4"):
                src = _grid(m, s4, kind, M.rand_grid(sd, kind, "a"))
                r = np.random.default_rng(M._seed("slice", sname, kind))
                D = r.uniform(-9, 9, dsh + ((3,) if kind == "vec4" else ())).astype(f32)
                DT = r.uniform(-9, 9, dsh).astype(f32) if kind == "vec4" else None
                for with_t in ((False, True) if kind == "vec4" else (False,)):
                    dst = s3.create(m.VecGrid if kind == "vec4" else m.RealGrid).from_numpy(D)
                    key = "slice/%s/%s%s" % (sname, kind, "/t" if with_t else "")
                    if kind == "real":
                        m.getSliceFrom4d(src=src, srct=srct, dst=dst)
                    elif with_t:
                        dstt = s3.create(m.RealGrid).from_numpy(DT)
                        m.getSliceFrom4dVec(src, srct, dst, dstt)
                        msg = M.same_as_fixture(GOLDEN, key + "/dstt", dstt.to_numpy())
                        assert msg is None, msg
                    else:
                        m.getSliceFrom4dVec(src, srct, dst)
                    msg = M.same_as_fixture(GOLDEN, key, dst.to_numpy())
                    assert msg is None, msg
        for shape in ("a", "c"):
            sd = M.SHAPES[shape]
            s4 = _solver(m, sd)
            V, R = M.rand_grid(sd, "vec4", "a"), M.rand_grid(sd, "real", "b")
            for c in range(4):
                v, r = _grid(m, s4, "vec4", V), _grid(m, s4, "real", R)
                m.getComp4d(v, r, c)
                msg = M.same_as_fixture(GOLDEN, "getComp/%s/%d" % (shape, c), r.to_numpy())
                assert msg is None and np.array_equal(v.to_numpy(), V), msg
                r.from_numpy(R)
                m.setComp4d(r, v, c)
                msg = M.same_as_fixture(GOLDEN, "setComp/%s/%d" % (shape, c), v.to_numpy())
                assert msg is None, msg


@pytest.mark.parametrize("kind", ("real", "vec4"))
def test_interpolation(hip_backend, kind):
    import manta as m
    fn = m.interpolateGrid4d if kind == "real" else m.interpolateGrid4dVec
    for rep in range(2):
        # up 4^4 -> 8^4 -> 16^4 and down again, each step reading the step before it
        src = _grid(m, _solver(m, M.INTERP_CHAIN[0][1]), kind, M.rand_grid(M.INTERP_CHAIN[0][1], kind, "chain"))
        for name, sd, td in M.INTERP_CHAIN:
            dst = _grid(m, _solver(m, td), kind, M.garbage(td, kind))
            fn(target=dst, source=src)
            msg = M.same_as_fixture(GOLDEN, "interp/%s/%s" % (name, kind), dst.to_numpy())
            assert msg is None, msg
            src = dst
        for name, (sd, td, kw) in M.INTERP_CASES.items():
            S = M.rand_grid(sd, kind, "interp")
            src, dst = _grid(m, _solver(m, sd), kind, S), _grid(m, _solver(m, td), kind, M.garbage(td, kind))
            fn(dst, src, **{k: m.vec4(*v) for k, v in kw.items()})
            msg = M.same_as_fixture(GOLDEN, "interp/%s/%s" % (name, kind), dst.to_numpy())
            assert msg is None, msg
            assert np.array_equal(src.to_numpy(), S)
    one = _grid(m, _solver(m, (4, 1, 4, 4)), kind)                 # an axis of one cell is below the precondition: refused, untouched
    with pytest.raises(RuntimeError) as err:
        fn(dst, one)
    assert "every axis of the source needs 2 cells" in str(err.value)
    with pytest.raises(RuntimeError):
        fn(dst, dst)


def _reduce_all(m, kind, arr, dims):
    g = _grid(m, _solver(m, dims, poison=False), kind, arr)
    return [np.float32(getattr(g, op)()) for op in ("getMin", "getMax", "getMaxAbs")]


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
@pytest.mark.parametrize("kind", M.KINDS)
def test_reductions_where_the_extremum_sits(hip_backend, kind, n):
    """the extremum in the first cell, the last cell, the tail past the last full block, tied, all cells equal, and a negative
    extremum for getMaxAbs; n cells in a row (the 4097 case: 17 blocks of 256 with one cell over)"""
    import manta as m
    dims = (n, 1, 1, 1) if n < 4097 else (241, 17, 1, 1)
    assert int(np.prod(dims)) == n
    base = M.rand_grid(dims, kind, "r")
    spots = sorted({0, n - 1, n - n % 256 if n % 256 and n > 256 else n // 2})
    variants = []
    for at in spots:
        for sign in (1, -1):
            a = base.copy()
            a.reshape(n, -1)[at] = sign * (97 if kind == "int" else 7.5)
            variants.append(a)
    tied = base.copy()
    tied.reshape(n, -1)[[0, n - 1]] = -97 if kind == "int" else -7.5
    variants += [tied, np.full_like(base, -3), np.zeros_like(base)]
    for a in variants:
        want = [M.reduction(kind, op, a) for op in ("getMin", "getMax", "getMaxAbs")]
        got = _reduce_all(m, kind, a, dims)
        assert [np.float32(w).tobytes() for w in want] == [g.tobytes() for g in got], (kind, n, want, got)
        b = M.rand_grid(dims, kind, "s")
        fn = {"real": m.grid4dMaxDiff, "int": m.grid4dMaxDiffInt, "vec3": m.grid4dMaxDiffVec3, "vec4": m.grid4dMaxDiffVec4}[kind]
        s = _solver(m, dims, poison=False)
        assert np.float32(fn(_grid(m, s, kind, a), _grid(m, s, kind, b))) == M.reduction(kind, "maxDiff", a, b)
        assert fn(_grid(m, s, kind, a), _grid(m, s, kind, a)) == 0.0


def test_sequence_of_the_grid4dop_script(hip_backend):
    """the computed branch of test_0032_grid4dop.py at its own size, against the values of the recorded reference run"""
    import manta as m
    s = _solver(m, M.SCRIPT32_DIMS)
    for kind, (c1, c2, add, mul, half) in M.SCRIPT32.items():
        V = (lambda x: x) if kind in ("real", "int") else (lambda x: m.vec3(x, x, x)) if kind == "vec3" else (lambda x: m.vec4(x, x, x, x))
        g1, g2, g3 = (_grid(m, s, kind) for _ in range(3))
        g1.setConst(V(c1))
        g2.setConst(V(c2))
        g3.setConst(V(9))
        g1.addConst(V(add))
        g2.multConst(V(mul))
        g3.copyFrom(g1)
        g3.add(g2)
        g3.addScaled(g2, V(half))
        want = GOLDEN["script32/" + kind]
        assert np.array_equal(want, M.script32_model()[kind])
        for g, w in zip((g1, g2, g3), want):
            a = g.to_numpy()
            assert a.dtype == want.dtype and (a.view(np.uint32) == np.array([w]).view(np.uint32)[0]).all(), (kind, w, a.flat[0])
    assert np.float32(g3.getMaxAbs()) == M.reduction("vec4", "getMaxAbs", np.full((1, 1, 1, 1, 4), want[2], f32))     # the script's "f3 3.9"


def test_sequence_of_the_interpol4d_script(hip_backend):
    """test_0042_interpol4d.py at res = 8: region, the four interpolations of each type, the display slices"""
    import manta as m
    res = M.SCRIPT42_RES
    sm, nm, xl = (res // 2,) * 4, (res,) * 4, (res * 2,) * 4
    S = {"sm": _solver(m, sm), "": _solver(m, nm), "xl": _solver(m, xl)}
    rs, re = sm[0] * 0.3, sm[0] * 0.7
    for kind, tag, value in (("real", "density", 1), ("vec4", "v3", m.vec4(1, 1, 1, 1))):
        interp = m.interpolateGrid4d if kind == "real" else m.interpolateGrid4dVec
        g = {"sm_" + tag: _grid(m, S["sm"], kind), tag: _grid(m, S[""], kind), "xl_" + tag: _grid(m, S["xl"], kind),
             tag + "2": _grid(m, S[""], kind), "sm_" + tag + "2": _grid(m, S["sm"], kind)}
        (m.setRegion4d if kind == "real" else m.setRegion4dVec4)(g["sm_" + tag], start=m.vec4(rs, rs, rs, rs), end=m.vec4(re, re, re, re), value=value)
        interp(target=g[tag], source=g["sm_" + tag])
        interp(target=g["xl_" + tag], source=g[tag])
        interp(target=g[tag + "2"], source=g["xl_" + tag])
        interp(target=g["sm_" + tag + "2"], source=g[tag + "2"])
        for name, grid in g.items():
            msg = M.same_as_fixture(GOLDEN, "script42/" + name, grid.to_numpy())
            assert msg is None, msg
            disp = grid.parent.create(m.RealGrid if kind == "real" else m.VecGrid)
            if kind == "real":
                m.getSliceFrom4d(src=grid, dst=disp, srct=int(grid.getSizeX() * 0.5))
            else:
                m.getSliceFrom4dVec(src=grid, dst=disp, srct=int(grid.getSizeX() * 0.5))
            msg = M.same_as_fixture(GOLDEN, "script42/slice_" + name, disp.to_numpy())
            assert msg is None, msg


def test_files_on_the_device(hip_backend, tmp_path):
    import manta as m
    dims = (4, 3, 2, 3)
    s = _solver(m, dims)
    g = _grid(m, s, "vec4")
    assert g.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid4d_vec4.uni")) == 1
    A = M.rand_grid(dims, "vec4", "file")
    assert np.array_equal(g.to_numpy(), A)
    for ext in ("uni", "raw"):
        name = str(tmp_path / ("g." + ext))
        g.save(name)
        h = _grid(m, s, "vec4", M.garbage(dims, "vec4"))
        h.load(name)
        assert np.array_equal(h.to_numpy(), A)


# ---- particle data -------------------------------------------------------------------------------------------------------------------
PD_CLASS = {"real": "PdataReal", "int": "PdataInt", "vec3": "PdataVec3"}


def _pd_system(m, n):
    """n live slots in channels of a larger capacity, everything past n filled with garbage that must stay"""
    s = m.Solver(name="s", gridSize=m.vec3(8, 7, 6), dim=3)
    parts = s.create(m.BasicParticleSystem)
    parts.resizeAll(n, n + 29)
    return s, parts


def _pd_channel(m, parts, kind, arr):
    pd = parts.create(getattr(m, PD_CLASS[kind]))
    pd.data.fill_(77)
    pd.from_numpy(arr)
    return pd


def _pd_tail_ok(pd):
    a = pd.data.cpu().numpy().reshape(pd._ncomp, pd.cap)
    return pd.cap > pd.size() and (a[:, pd.size():] == 77).all()


def _pd_run(m, parts, key, n, kind, op):
    a, b, t = M.pd_inputs(key, n, kind, op)
    A, B = _pd_channel(m, parts, kind, a), _pd_channel(m, parts, kind, b)
    T = None if t is None else _pd_channel(m, parts, "int", t)
    V = (lambda v: v) if kind != "vec3" else (lambda v: m.vec3(*v))
    what = op.split("/")[0]
    if what in ("add", "sub", "mult", "safeDiv"):
        getattr(A, what)(B)
    elif what in ("addConst", "multConst"):
        getattr(A, what)(V(M.PD_CONST[kind]))
    elif what == "addScaled":
        A.addScaled(B, V(M.PD_FACTOR[kind]))
    elif what == "clamp":
        A.clamp(*M.PD_CLAMP[kind])
    elif what == "clampMin":
        A.clampMin(M.PD_CLAMP[kind][0])
    elif what == "clampMax":
        A.clampMax(M.PD_CLAMP[kind][1])
    elif what == "setConstRange":
        A.setConstRange(V(M.PD_CONST[kind]), *M.pd_range(n))
    elif what == "setConstIntFlag":
        A.setConstIntFlag(V(M.PD_CONST[kind]), T, M.PD_FLAG)
    elif what in M.PD_MINMAX:
        r = np.array([getattr(A, what)()], f32)
    elif what == "sum":
        r = A.sum() if T is None else A.sum(T, M.PD_FLAG)
        r = np.array([r], np.int32) if kind == "int" else np.array(list(r) if kind == "vec3" else [r], f32)
    else:
        r = np.array([getattr(A, what)()], f32)
    assert _pd_tail_ok(A) and _pd_tail_ok(B) and np.array_equal(B.to_numpy(), b)
    if op in M.PD_ARRAY_OPS:
        return A.to_numpy()
    assert np.array_equal(A.to_numpy(), a)
    return r


@pytest.mark.parametrize("kind", M.PD_KINDS)
@pytest.mark.parametrize("n", M.PD_SIZES)
def test_pdata_methods(hip_backend, n, kind, capsys):
    """every method at this size: arrays and extrema equal the reference bit for bit; the sums are bit-identical to the reference's on
    the exactly summable inputs and inside gamma(n-1) * sum|term| + 2^-24 |S| of the exact sum on the random ones (the reference's own
    one-thread sum meets the same bound: tests/test_grid4d_model.py); the same bits on a second run"""
    import manta as m
    _pd_run(m, _pd_system(m, 6000)[1], "pd/6000/%s/sum" % kind, 6000, kind, "sum")            # a larger system first
    s, parts = _pd_system(m, n)
    worst = 0.0
    for key, nn, k, op in M.pd_cases():
        if nn != n or k != kind:
            continue
        got = [_pd_run(m, parts, key, n, kind, op) for _ in range(2)]
        assert got[0].tobytes() == got[1].tobytes(), key
        if op not in M.PD_SUMS or kind == "int" and op.split("/")[0] == "sum" or key.startswith("pdx/"):
            msg = M.same_as_fixture(GOLDEN, key, got[0])
            assert msg is None, msg
            continue
        a, b, t = M.pd_inputs(key, n, kind, op)
        exact, bound = M.pd_sum_bound(M.pd_terms(kind, op, a, t))
        err = np.abs(got[0].astype(np.float64) - exact)
        share = float((err / np.where(bound > 0, bound, 1)).max()) if err.size else 0.0
        print("%s: error %.3g, %.4f of the bound" % (key, float(err.max()) if err.size else 0.0, share))
        assert (err <= bound).all(), (key, err, bound)
        worst = max(worst, share)
    with capsys.disabled():
        print("\n  pdata %s n=%d: largest sum error as a share of the bound %.4f" % (kind, n, worst))


def test_pdata_files_on_the_device(hip_backend, tmp_path):
    import manta as m
    s, parts = _pd_system(m, 37)
    v = _pd_channel(m, parts, "vec3", np.zeros((37, 3), f32))
    assert v.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid4d_pdata_vec3.uni")) == 1
    A = M.pd_rand(37, "vec3", "file")
    assert np.array_equal(v.to_numpy(), A) and _pd_tail_ok(v)
    for kind in M.PD_KINDS:
        a = _pd_channel(m, parts, kind, M.pd_rand(37, kind, "file"))
        name = str(tmp_path / ("p_%s.uni" % kind))
        a.save(name)
        b = _pd_channel(m, parts, kind, M.pd_rand(37, kind, "other"))
        b.load(name)
        assert np.array_equal(b.to_numpy(), M.pd_rand(37, kind, "file")) and _pd_tail_ok(b)


# ---- the harness helpers -----------------------------------------------------------------------------------------------------------------
def test_check_symmetry_and_init_grid_with_pos(hip_backend):
    """every recorded case of checkSymmetry / checkSymmetryVec3 (even and odd sizes, 2-D and 3-D, each axis, with and without err,
    symmetrize, bound, disabled sweeps), after a call on a larger solver, twice; err and pool storage start from garbage"""
    import manta as m
    D = M.sym_digests(GOLDEN)
    big = m.Solver(name="big", gridSize=m.vec3(40, 9, 7), dim=3)
    m.checkSymmetryVec3(big.create(m.MACGrid), big.create(m.RealGrid), symmetrize=True, axis=2)
    solvers = {}
    for shape, axis, sym, bound in M.SYM_CASES:
        dims = M.SYM_SHAPES[shape]
        s = solvers.setdefault(shape, m.Solver(name=shape, gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2))
        for vec in (False, True):
            for dis in (M.SYM_DISABLE if vec else (0,)):
                for with_err in (True, False):
                    for rep in range(2):
                        a = s.create(m.MACGrid if vec else m.RealGrid).from_numpy(M.sym_input(shape, vec))
                        err = s.create(m.RealGrid).from_numpy(np.full((dims[2], dims[1], dims[0]), 7.0 if vec else np.nan, f32)) if with_err else None
                        if vec:
                            m.checkSymmetryVec3(a=a, err=err, symmetrize=sym, axis=axis, bound=bound, disable=dis)
                        else:
                            m.checkSymmetry(a=a, err=err, symmetrize=sym, axis=axis, bound=bound)
                        key = M.sym_key(shape, axis, sym, bound, vec, dis, with_err)
                        assert M.sha(a.to_numpy()) == D[key], (key, rep)
                        if with_err:
                            assert M.sha(err.to_numpy()) == D[key + "/err"], (key, rep)
    for shape, dims in M.SYM_SHAPES.items():
        g = solvers[shape].create(m.RealGrid).from_numpy(np.full((dims[2], dims[1], dims[0]), np.nan, f32))
        m.testInitGridWithPos(g)
        msg = M.same_as_fixture(GOLDEN, "initpos/" + shape, g.to_numpy())
        assert msg is None, msg


def test_set_noise_pdata(hip_backend):
    """5000 particles inside the domain, on cell faces and centres, at negative positions and far outside the 128-cell tile period:
    the three plugins equal the recorded reference bit for bit, and the package's own numpy models of the noise field"""
    import manta as m
    import obstacle_model
    import turbulence_model
    pos = M.noise_positions()
    s = m.Solver(name="n", gridSize=m.vec3(*M.NOISE_DIMS), dim=3)
    noise = s.create(m.NoiseField, fixedSeed=265)
    parts = s.create(m.BasicParticleSystem)
    ch = {k: parts.create(getattr(m, PD_CLASS[k])) for k in M.PD_KINDS}
    parts.set_positions(pos)
    parts.reserve(M.NOISE_N + 100)
    assert parts.cap > parts.np == M.NOISE_N
    fns = {"real": m.setNoisePdata, "int": m.setNoisePdataInt, "vec3": m.setNoisePdataVec3}
    tile, params = noise._tile.detach().cpu().numpy(), np.array(list(noise._params()), f32)
    for rep in range(2):
        for kind, pd in ch.items():
            pd.data.fill_(77)
            fns[kind](parts, pd, noise, M.NOISE_SCALE[kind])
            got = pd.to_numpy()
            msg = M.same_as_fixture(GOLDEN, "noise/" + kind, got)
            assert msg is None, msg
            assert _pd_tail_ok(pd)
            if kind == "vec3":
                want = turbulence_model.evaluate_vec(tile, params, pos, 0) * f32(M.NOISE_SCALE[kind])
            else:
                want = obstacle_model.noise_evaluate(tile.reshape(-1), params, pos[:, 0], pos[:, 1], pos[:, 2]) * f32(M.NOISE_SCALE[kind])
                want = want.astype(f32) if kind == "real" else np.trunc(want).astype(np.int32)
            assert np.array_equal(got, np.asarray(want).reshape(got.shape).astype(got.dtype))
    assert np.array_equal(parts.get_positions(), pos)
    empty = s.create(m.BasicParticleSystem)
    m.setNoisePdata(empty, empty.create(m.PdataReal), noise)                   # no slot, no launch


@pytest.mark.parametrize("case", sorted(M.ADDPARTS))
def test_add_test_parts(hip_backend, case):
    import manta as m
    I = M.addparts_inputs(case)
    s = m.Solver(name="s", gridSize=m.vec3(*M.ADDPARTS_DIMS), dim=3)
    parts = s.create(m.BasicParticleSystem)
    ch = dict(real=parts.create(m.PdataReal), vec=parts.create(m.PdataVec3), ints=parts.create(m.PdataInt), plain=parts.create(m.PdataReal))
    src_real, src_mac = s.create(m.RealGrid).from_numpy(I["src_real"]), s.create(m.MACGrid).from_numpy(I["src_mac"])
    ch["real"].setSource(src_real)
    ch["vec"].setSource(src_mac, isMAC=True)
    parts.set_positions(I["pos"], I["flags"])
    for k, pd in ch.items():
        pd.from_numpy(I[k])
    m.addTestParts(parts, I["num"])
    got = dict(pos=parts.get_positions(), flags=parts.get_flags(), **{k: pd.to_numpy() for k, pd in ch.items()})
    for k, v in got.items():
        msg = M.same_as_fixture(GOLDEN, "addparts/%s/%s" % (case, k), v)
        assert msg is None, msg


def test_sequence_of_the_pdataop_script(hip_backend):
    """test_0500_pdataop.py's computed branch on the ten particles addTestParts makes, against the values of the recorded reference run
    (the same arithmetic as the 4-D grid script's, on channels)"""
    import manta as m
    s = m.Solver(name="main", gridSize=m.vec3(12, 19, 31), dim=3)
    pp = s.create(m.BasicParticleSystem)
    ch = {k: [pp.create(getattr(m, PD_CLASS[k])) for _ in range(3)] for k in M.PD_KINDS}
    m.addTestParts(pp, 10)
    assert pp.pySize() == 10 and (pp.get_flags() == M.PNEW).all() and not pp.get_positions().any()
    for kind, (g1, g2, g3) in ch.items():
        c1, c2, add, mul, half = M.SCRIPT32[kind]
        V = (lambda x: x) if kind != "vec3" else (lambda x: m.vec3(x, x, x))
        g1.setConst(V(c1))
        g2.setConst(V(c2))
        g3.setConst(V(9))
        g1.addConst(V(add))
        g2.multConst(V(mul))
        g3.copyFrom(g1)
        g3.add(g2)
        g3.addScaled(g2, V(half))
        want = GOLDEN["script500/" + kind]
        for g, w in zip((g1, g2, g3), want):
            a = g.to_numpy()
            assert a.shape[0] == 10 and (a.view(np.uint32) == np.array([w]).view(np.uint32)[0]).all(), (kind, w, a.flat[0])


# ---- the loops of the two remaining harness scripts, restated, against runs of the compiled reference (tools/record_grid4d.py).
# The pressure solve is the one thing in them that the device does not reproduce bit for bit (another summation order inside the
# preconditioner and the dot products); the project's parity bound for it is 1e-5 of the largest magnitude (smoke(), the pressure
# tests).  Everything downstream of a solve is held to a bound derived from that one, written where it is used; everything
# upstream of it, and the iteration counts, are held exactly. ----
def _rel(got, want):
    return float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max() / max(float(np.abs(want).max()), 1e-30))


def _norms(a):
    return np.array([np.abs(a).max(), np.abs(a.astype(np.float64)).sum()], np.float64)


@pytest.mark.parametrize("dim", (2, 3))
def test_loop_of_the_symmetric_advection_script(hip_backend, dim, capsys):
    """test_2005_symmAdv.py at res = 12 with 2 steps per field, every direction, against the recorded reference run:
    - CG iterations: equal;
    - pressure and velocity after the solve and the symmetrising: 1e-5 relative (the solve's parity bound; symmetrising copies values);
      in 3-D, where the fixture keeps their largest magnitude and fp64 sum of magnitudes, those to 1e-5 relative;
    - the first symmetry errors (differences of two such values): 2e-5 of the field's largest magnitude;
    - the final error grids: the script's own doTestGrid threshold, 1e-5 in the largest difference;
    - the final phi: |grad phi| = 1 and a velocity off by at most 1e-5 * 2 moves each of the three traces of a MacCormack step by
      2e-5 cells, two steps: 2 * 3 * 2e-5 = 1.2e-4, bound 2e-4 absolute;
    - the final velocity: the same traces through a field that changes by up to 2 per cell at the box's faces, plus its own 2e-5:
      2 * (3 * 2 * 2e-5 + 2e-5) = 2.8e-4, bound 4e-4 absolute"""
    import manta as m
    res, steps = M.LOOP2005["res"], M.LOOP2005["steps"]
    gs = m.vec3(res, res, res if dim == 3 else 1)
    s = m.Solver(name="main", gridSize=gs, dim=dim)
    s.timestep = 1.0
    errR1, errV1, errR2, errV2, rhs, pressure = (s.create(m.RealGrid) for _ in range(6))
    flags, vel, phi = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.LevelsetGrid)
    drop = s.create(m.Sphere, center=gs * m.vec3(0.5, 0.5, 0.5), radius=res * 0.25)
    dirs_symm = [0, 2, 1, 2, 1, 0]
    dirs_vel = [m.vec3(0, 2, 0), m.vec3(0, -2, 0), m.vec3(2, 0, 0), m.vec3(-2, 0, 0), m.vec3(0, 0, 2), m.vec3(0, 0, -2)]
    off = 1.25 if dim == 2 else 0.0
    report = []
    for symms in range(2 * dim):
        key = "loop2005/%d/%d/" % (dim, symms)
        flags.initDomain(boundaryWidth=0)
        for g in (errR1, errV1, pressure, rhs):
            g.setConst(0)
        phi.setConst(1e10)
        phi.join(drop.computeLevelset())
        flags.fillGrid()
        vel.setConst(m.vec3(0, 0, 0))
        dir1, dir2 = dirs_symm[symms - symms % 2], dirs_symm[symms - symms % 2 + 1]
        s.create(m.Box, p0=gs * m.vec3(0.30, 0.30, 0.30 - off), p1=gs * m.vec3(0.70, 0.70, 0.70 + off)).applyToGrid(grid=vel, value=dirs_vel[symms])
        m.solvePressure(flags=flags, vel=vel, pressure=pressure, cgMaxIterFac=99., cgAccuracy=1e-3, retRhs=rhs)
        assert m.lastCgStats()["iterations"] == int(GOLDEN[key + "iterations"][0]), key
        m.checkSymmetry(a=pressure, err=errR1, axis=dir1)
        m.checkSymmetryVec3(a=vel, err=errV1, axis=dir1)
        first = np.array([errR1.getMax(), errV1.getMax()], f32)
        axes = (dir1, dir2) if dim == 3 else (dir1,)
        for ax, eR, eV in zip(axes, (errR1, errR2), (errV1, errV2)):
            m.checkSymmetry(a=pressure, symmetrize=True, axis=ax)
            m.checkSymmetryVec3(a=vel, symmetrize=True, axis=ax)
            m.checkSymmetry(a=pressure, err=eR, axis=ax)
            m.checkSymmetryVec3(a=vel, err=eV, axis=ax)
            assert eR.getMax() == 0.0 and eV.getMax() == 0.0              # symmetrised: exactly symmetric
        ps, vs = pressure.to_numpy(), vel.to_numpy()
        s.create(m.Box, p0=gs * m.vec3(0.4, 0.4, 0.4 - off), p1=gs * m.vec3(0.6, 0.6, 0.6 + off)).applyToGrid(grid=flags, value=m.FlagObstacle)
        for t in range(steps):
            for ax in axes:
                m.checkSymmetry(a=phi, symmetrize=True, axis=ax)
            phi.setBoundNeumann(0)
            m.advectSemiLagrange(flags=flags, vel=vel, grid=phi, order=2, clampMode=1)
            for ax, eR in zip(axes, (errR1, errR2)):
                m.checkSymmetry(a=phi, err=eR, axis=ax)
            s.step()
        for t in range(steps):
            phi.setBoundNeumann(0)
            for ax in axes:
                m.checkSymmetryVec3(a=vel, symmetrize=True, axis=ax)
            m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2, clampMode=1)
            for ax, eV in zip(axes, (errV1, errV2)):
                m.checkSymmetryVec3(a=vel, err=eV, axis=ax)
            s.step()
        got_err = np.stack([g.to_numpy() for g in (errR1, errR2, errV1, errV2)])
        if dim == 2:
            got_err[[1, 3]] = 0                        # the 2-D script never writes errR2 / errV2; the recorded run's are fresh grids
        pmax, vmax = float(GOLDEN[key + "pressureSym/norms"][0]), float(GOLDEN[key + "velSym/norms"][0])
        figs = dict(
            pressure=_rel(ps, GOLDEN[key + "pressureSym"]) if dim == 2 else float(np.abs(_norms(ps) / GOLDEN[key + "pressureSym/norms"] - 1).max()),
            velocity=_rel(vs, GOLDEN[key + "velSym"]) if dim == 2 else float(np.abs(_norms(vs) / GOLDEN[key + "velSym/norms"] - 1).max()),
            firstR=abs(float(first[0]) - float(GOLDEN[key + "first"][0])) / pmax, firstV=abs(float(first[1]) - float(GOLDEN[key + "first"][1])) / vmax,
            err=float(np.abs(got_err - GOLDEN[key + "err"]).max()), phi=float(np.abs(phi.to_numpy() - GOLDEN[key + "phi"]).max()),
            vel=float(np.abs(vel.to_numpy() - GOLDEN[key + "vel"]).max()) if dim == 2 else float(np.abs(_norms(vel.to_numpy()) / GOLDEN[key + "vel/norms"] - 1).max()))
        report.append("  %s %s" % (key, " ".join("%s %.3g" % kv for kv in figs.items())))
        bounds = dict(pressure=1e-5, velocity=1e-5, firstR=2e-5, firstV=2e-5, err=1e-5, phi=2e-4, vel=4e-4)
        for k, b in bounds.items():
            assert figs[k] <= b, (key, k, figs[k], b, report)
    with capsys.disabled():
        print("\n" + "\n".join(report))


def test_loop_of_the_particle_io_script(hip_backend, tmp_path, capsys):
    """test_2065_partIo.py at res = 16 against the recorded reference run of its generate branch, then its check branch.
    - the sampled positions (before any solve): bit for bit; the noise channel (evaluated at them): bit for bit; CG iterations: equal;
    - positions after 5 RK4 steps of dt 0.58 through a velocity within 1e-5 * vmax of the reference's: each step adds dt * 1e-5 * vmax
      and at most doubles what is there (dt * |grad vel| < 1 here), so 5 steps stay below 2 * 5 * 0.58 * 1e-5 * vmax, plus 1e-5 for
      fp32 rounding of coordinates up to 16;
    - the mapped density: the script's own doTestGrid threshold, 1e-5 in the largest difference;
    - check branch: the saved positions and channel, loaded into a fresh system, map to the same density bit for bit"""
    import manta as m
    res = M.LOOP2065["res"]
    gs = m.vec3(res, res, res)

    def stage():
        s = m.Solver(name="main", gridSize=gs, dim=3)
        s.timestep = 0.58
        flags, vel, pressure, density = m.FlagGrid(parent=s), m.MACGrid(parent=s), m.RealGrid(parent=s), m.RealGrid(parent=s)
        pp = m.BasicParticleSystem(parent=s)
        return s, flags, vel, pressure, density, pp, pp.create(m.PdataVec3), pp.create(m.PdataReal)
    s, flags, vel, pressure, density, pp, pVel, pDens = stage()
    flags.initDomain(boundaryWidth=0)
    noise = m.NoiseField(parent=s, fixedSeed=M.LOOP2065["fixedSeed"])       # the script's has no fixed seed: its offset depends on the process
    noise.posScale = m.vec3(100)
    noise.clamp, noise.clampNeg, noise.clampPos, noise.valScale, noise.valOffset, noise.timeAnim = True, 0, 1.2, 0.9, 0.15, 0.1
    phiInit = m.Box(parent=s, p0=gs * m.vec3(0.2, 0.2, 0.2), p1=gs * m.vec3(0.8, 0.4, 0.8)).computeLevelset()
    phiInit.join(m.Box(parent=s, p0=gs * m.vec3(0.2, 0.6, 0.2), p1=gs * m.vec3(0.8, 0.8, 0.8)).computeLevelset())
    flags.updateFromLevelset(phiInit)
    m.sampleFlagsWithParticles(flags=flags, parts=pp, discretization=3, randomness=0.2)
    n, iterations = (int(v) for v in GOLDEN["loop2065/count"])
    assert pp.pySize() == n and M.sha(pp.get_positions()) == str(GOLDEN["loop2065/pos0#sha"])
    pDens.setConst(1.3)
    flags.fillGrid()
    m.mapPartsToGrid(target=density, flags=flags, parts=pp, source=pDens)
    m.addBuoyancy(density=density, vel=vel, gravity=m.vec3(0, -5e-1, 0), flags=flags)
    m.setWallBcs(flags=flags, vel=vel)
    m.solvePressure(flags=flags, vel=vel, pressure=pressure)
    assert m.lastCgStats()["iterations"] == iterations
    m.setWallBcs(flags=flags, vel=vel)
    vmax = float(GOLDEN["loop2065/velMax"][0])
    assert abs(float(np.abs(vel.to_numpy()).max()) - vmax) <= 1e-5 * vmax
    m.setNoisePdata(pp, pDens, noise)
    every = M.LOOP2065["every"]
    assert np.array_equal(pDens.to_numpy()[::every], GOLDEN["loop2065/pDens/sample"]) and M.sha(pDens.to_numpy()) == str(GOLDEN["loop2065/pDens#sha"])
    for t in range(5):
        pp.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4, deleteInObstacle=False)
        s.step()
    assert pp.pySize() == n
    pos = pp.get_positions()
    dpos = float(np.abs(pos[::every].astype(np.float64) - GOLDEN["loop2065/pos1/sample"]).max())
    density.setConst(-1.)
    m.mapPartsToGrid(target=density, flags=flags, parts=pp, source=pDens)
    ddens = float(np.abs(density.to_numpy() - GOLDEN["loop2065/density"]).max())
    with capsys.disabled():
        print("\n  loop2065: positions off by at most %.3g (bit-identical: %s), density by %.3g" % (dpos, M.sha(pos) == str(GOLDEN["loop2065/pos1#sha"]), ddens))
    assert dpos <= 2 * 5 * 0.58 * 1e-5 * vmax + 1e-5
    assert M.sha(pos) == str(GOLDEN["loop2065/pos1#sha"])          # what the issue asks of the positions: bit for bit
    assert ddens <= 1e-5
    pp.save(str(tmp_path / "parts.uni"))
    pDens.save(str(tmp_path / "pDens.uni"))
    s2, flags2, vel2, pressure2, density2, pp2, pVel2, pDens2 = stage()
    flags2.initDomain(boundaryWidth=0)
    flags2.fillGrid()
    pp2.load(str(tmp_path / "parts.uni"))
    pDens2.load(str(tmp_path / "pDens.uni"))
    m.mapPartsToGrid(target=density2, flags=flags2, parts=pp2, source=pDens2)
    assert pp2.get_positions().tobytes() == pos.tobytes() and np.array_equal(pp2.get_flags(), pp.get_flags())
    assert pDens2.to_numpy().tobytes() == pDens.to_numpy().tobytes() and pVel2.size() == n
    assert density2.to_numpy().tobytes() == density.to_numpy().tobytes()
