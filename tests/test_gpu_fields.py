"""GPU: the fire, wave-equation and uv-grid plugins through the package on the HIP backend against the numpy model and the recorded
reference (tests/golden/fields.npz; how each array was produced: tools/record_fields.py; arrays of more than fields_model.FULL_LIMIT
elements are in the fixture as SHA-256 digests, so the device result is also compared, word by word, with the model's array).

HIP = model bit for bit everywhere.  HIP = reference bit for bit as well, except `flame` and `heat`: the reference computes
pow(x, 0.5f) with glibc's powf, the device the correctly rounded square root, so flame is held to 1 ulp and heat to
(ignitionTemp + maxTemp) * ulp(flame) plus one rounding, in the cells the fixture lists, and to equality everywhere else.

Grids: 7x5x4, 6x6x6, 33x31x29 (odd rows, partial wavefronts, several blocks), 12x9x1 (2-D), 3x3x1 (one interior cell).  Outputs are
pre-filled with the fixture's caller values and, in a second call, with NaN; the solver's pool scratch is pre-filled with NaN (floats)
and with 2 (ints: a value the extrapolation passes compare against)."""
import os

import numpy as np
import pytest

import fields_model as M
import util

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fields.npz"))
f32, f64 = np.float32, np.float64


def _solver(m, dims, dt=1.0):
    s = m.Solver(name="t", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)
    s.timestep = dt
    return s


def _grid(s, cls, arr):
    g = s.create(cls)
    g.from_numpy(arr)
    return g


def _poison_pool(s):
    """the next scratch grids the plugins take from the solver's pool hold NaN (floats) or 2 (ints)"""
    import torch
    for kind, ncomp in (("real", 1), ("vec", 3)):
        for _ in range(2):
            s._pool.setdefault(kind, []).append(torch.full((ncomp * s.ncells,), float("nan"), dtype=torch.float32, device=s.device))
    for _ in range(2):
        s._pool.setdefault("int", []).append(torch.full((s.ncells,), 2, dtype=torch.int32, device=s.device))


def bits_equal(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    d = got.view(np.uint32) != want.view(np.uint32)
    assert not d.any(), "%s: %d of %d words differ, first at %s" % (tag, int(d.sum()), d.size, np.argwhere(d)[0])


def check(key, got, model):
    """HIP = model (word by word) and HIP = fixture (the array or its digest)"""
    bits_equal(key + " vs model", got, model)
    msg = M.same_as_fixture(GOLDEN, key, got)
    assert msg is None, msg


def check_near(key, got, model, bound):
    """HIP = model word by word; HIP = reference except in the recorded cells, where it is within `bound`"""
    bits_equal(key + " vs model", got, model)
    msg, idx, ref = M.near_fixture(GOLDEN, key, got)
    assert msg is None, msg
    err = np.abs(got.reshape(-1)[idx].astype(f64) - ref.astype(f64))
    print("%s: %d cells differ from the reference, largest error %.3g" % (key, idx.size, err.max() if idx.size else 0.0))
    assert (err <= np.broadcast_to(bound, got.shape).reshape(-1)[idx]).all(), key


# ---------------------------------------------------------------------------------------------------------------------------------
# fire
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(M.FIRE_CASES))
def test_process_burn_and_update_flame(hip_backend, case):
    import manta as m
    name, absent, par = M.FIRE_CASES[case]
    dims = M.DIMS[name]
    I = M.fire_inputs(name)
    model, mflame = M.run_fire(case)
    s = _solver(m, dims, M.FIRE_DT)
    g = {k: _grid(s, m.RealGrid, v) for k, v in I.items()}
    kw = {k: g[k] for k in M.OPTIONAL if k not in absent}
    _poison_pool(s)
    live = s._live
    m.processBurn(fuel=g["fuel"], density=g["density"], react=g["react"], burningRate=par["burningRate"], flameSmoke=par["flameSmoke"],
                  ignitionTemp=par["ignitionTemp"], maxTemp=par["maxTemp"], flameSmokeColor=m.vec3(*par["color"]), **kw)
    assert s._live == live                                  # one kernel, no scratch
    for k in ("fuel", "density", "react", "red", "green", "blue"):
        if k in absent:
            bits_equal(k + " untouched", g[k].to_numpy(), I[k])
        else:
            check("fire/%s/%s" % (case, k), g[k].to_numpy(), model[k])
    if "heat" in absent:
        bits_equal("heat untouched", g["heat"].to_numpy(), I["heat"])
    else:
        heat = g["heat"].to_numpy()
        check_near("fire/%s/heat" % case, heat, model["heat"], M.heat_bound(M.fire_flame(case), heat, par["ignitionTemp"], par["maxTemp"]))
    interior = M.interior_mask(M.shape_of(dims))
    assert name == "g3" or (g["density"].to_numpy()[interior] > 1).any()          # not clamped
    for fill in ("fixture", "nan"):
        flame = _grid(s, m.RealGrid, M.prefill(name, "flame") if fill == "fixture" else np.full(M.shape_of(dims), np.nan, f32))
        m.updateFlame(react=g["react"], flame=flame)
        got = flame.to_numpy()
        if fill == "fixture":
            check_near("fire/%s/flame" % case, got, mflame, M.ulp(got).astype(f64))
        else:
            bits_equal("flame interior", got[interior], mflame[interior])
            assert np.isnan(got[~interior]).all()           # border cells keep the caller's values


def test_flame_special_values(hip_backend):
    """pow(x, 0.5f)'s special cases on the device: -0 -> +0 (heat untouched), a negative react -> NaN in heat; updateFlame: react <= 0
    and NaN -> 0"""
    import manta as m
    s = _solver(m, (6, 3, 1), 0.4)
    sh = (1, 3, 6)
    fuel, dens, heat = np.full(sh, 0.9, f32), np.full(sh, 0.1, f32), np.full(sh, 5, f32)
    react = np.zeros(sh, f32)
    react[0, 1, 1:5] = (-0.0, -0.25, np.inf, 0.25)
    g = [_grid(s, m.RealGrid, a) for a in (fuel, dens, react, heat)]
    m.processBurn(fuel=g[0], density=g[1], react=g[2], heat=g[3])
    model = M.process_burn(fuel, dens, react, None, None, None, heat, 0.4)
    h = g[3].to_numpy()
    assert h[0, 1, 1] == 5 and np.isnan(h[0, 1, 2]) and np.isnan(h[0, 1, 3]) and np.isfinite(h[0, 1, 4])
    assert np.array_equal(np.isnan(h), np.isnan(model["heat"]))
    bits_equal("heat", np.nan_to_num(h, nan=-1.0), np.nan_to_num(model["heat"], nan=-1.0))
    bits_equal("react", g[2].to_numpy(), model["react"])
    src = np.zeros(sh, f32)
    src[0, 1, 1:5] = (-0.0, -4.0, np.nan, 4.0)
    flame = _grid(s, m.RealGrid, np.full(sh, 3, f32))
    m.updateFlame(react=_grid(s, m.RealGrid, src), flame=flame)
    assert flame.to_numpy()[0, 1, 1:5].tolist() == [0.0, 0.0, 0.0, 2.0] and not np.signbit(flame.to_numpy()[0, 1, 1])


# ---------------------------------------------------------------------------------------------------------------------------------
# wave equation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.ALL)
def test_calc_sec_deriv_2d(hip_backend, name):
    import manta as m
    dims = M.DIMS[name]
    s = _solver(m, dims)
    v = M.secderiv_input(name)
    interior = M.interior_mask(v.shape)
    gv = _grid(s, m.RealGrid, v)
    for fill in ("fixture", "nan"):
        curv = _grid(s, m.RealGrid, M.prefill(name, "curv") if fill == "fixture" else np.full(v.shape, np.nan, f32))
        m.calcSecDeriv2d(gv, curv)
        got = curv.to_numpy()
        model = M.sec_deriv_2d(v, M.prefill(name, "curv"))
        if fill == "fixture":
            check("secderiv/" + name, got, model)
        else:
            bits_equal("interior", got[interior], model[interior])
            assert np.isnan(got[~interior]).all()
    bits_equal("v", gv.to_numpy(), v)
    with pytest.raises(RuntimeError, match="must not alias"):
        m.calcSecDeriv2d(gv, gv)


@pytest.mark.parametrize("name", M.ALL)
def test_total_sum_and_normalize(hip_backend, name):
    """exactly summable inputs: the sum and the normalised grid are the reference's bit for bit, whatever the order of additions.
    Random inputs: any order of fp64 additions moves the sum by at most (n-1) 2^-53 sum|h|, far below half an fp32 ulp, so the fp32
    sum is within 1 ulp of the reference's; the factor then is within 1 ulp and each product rounds once more: 2 ulp per cell."""
    import manta as m
    dims = M.DIMS[name]
    s = _solver(m, dims)
    for kind in M.SUM_KINDS:
        h = M.sum_input(name, kind)
        g = _grid(s, m.RealGrid, h)
        _poison_pool(s)
        got_sum = f32(m.totalSum(height=g))
        bits_equal("h after totalSum", g.to_numpy(), h)
        m.normalizeSumTo(g, M.SUM_TARGET)
        got = g.to_numpy()
        ref_sum = GOLDEN["sum/%s/%s/sum" % (name, kind)][0]
        print("sum/%s/%s: sum %r (reference %r), margin of any order %.3g, ulp %.3g" % (name, kind, got_sum, ref_sum, M.sum_margin(h), M.ulp(ref_sum)))
        if kind == "exact":
            assert got_sum.tobytes() == ref_sum.tobytes()
            check("sum/%s/exact/grid" % name, got, M.normalize_sum_to(h, M.SUM_TARGET))
        else:
            assert abs(f64(got_sum) - f64(ref_sum)) <= M.ulp(ref_sum)
            model = M.normalize_sum_to(h, M.SUM_TARGET)          # the reference's grid, bit for bit (tests/test_fields_model.py)
            assert M.same_as_fixture(GOLDEN, "sum/%s/random/grid" % name, model) is None
            err = np.abs(got.astype(f64) - model.astype(f64)) / M.ulp(model).astype(f64)
            print("    grid: largest error %.3g ulp" % err.max())
            assert (err <= 2).all()


@pytest.mark.parametrize("crankNic", (False, True))
@pytest.mark.parametrize("name", M.ALL)
def test_wave_system_kernel(hip_backend, name, crankNic):
    """the set-up kernel of cgSolveWE after the existing mf_make_laplace_matrix, through the C ABI: matrix and right-hand side"""
    import manta as m
    dims = M.DIMS[name]
    I = M.wave_inputs(name)
    s = _solver(m, dims, M.WAVE_DT)
    flags, ut, utm1 = _grid(s, m.FlagGrid, I["flags"]), _grid(s, m.RealGrid, I["ut"]), _grid(s, m.RealGrid, I["utm1"])
    A = [s.create(m.RealGrid) for _ in range(4)]
    rhs = _grid(s, m.RealGrid, np.full(I["ut"].shape, np.nan, f32))
    sx, sy, sz = dims
    s.lib.call("mf_make_laplace_matrix", sx, sy, sz, flags.ptr, A[0].ptr, A[1].ptr, A[2].ptr, A[3].ptr, None, s.stream)
    s.lib.call("mf_fields_wave_system", sx, sy, sz, A[0].ptr, A[1].ptr, A[2].ptr, A[3].ptr, rhs.ptr, ut.ptr, utm1.ptr,
               float(M.wave_s(M.WAVE_DT, M.WAVE_CSQR)), int(crankNic), s.stream)
    model = M.run_wave_system(name, crankNic)
    for k, g in zip(("A0", "Ai", "Aj", "Ak", "rhs"), A + [rhs]):
        check("wavesys/%s/%d/%s" % (name, crankNic, k), g.to_numpy(), model[k])
    bits_equal("ut", ut.to_numpy(), I["ut"])


@pytest.mark.parametrize("crankNic", (False, True))
@pytest.mark.parametrize("name", sorted(M.CG_DIMS))
def test_cg_solve_we(hip_backend, name, crankNic):
    """the same iteration count as the recorded reference; ut within 1e-5 relative, the bound test_gpu_parity.py::test_cg_solve_diffusion
    uses for the same solver; utm1 is the old ut, out the new one"""
    import manta as m
    I = M.cg_inputs(name)
    s = _solver(m, I["dims"], M.CG_DT)
    flags, ut, utm1 = _grid(s, m.FlagGrid, I["flags"]), _grid(s, m.RealGrid, I["ut"]), _grid(s, m.RealGrid, I["utm1"])
    out = _grid(s, m.RealGrid, np.full(I["ut"].shape, np.nan, f32))
    _poison_pool(s)
    m.cgSolveWE(flags=flags, ut=ut, utm1=utm1, out=out, crankNic=crankNic, cSqr=M.CG_CSQR)
    key = "cgwe/%s/%d" % (name, crankNic)
    stats = m.lastCgStats()
    want = GOLDEN[key + "/ut"]
    e = util.rel_err(ut.to_numpy(), want)
    print("%s: iterations %d (reference %d), ut rel. error %.3g" % (key, stats["iterations"], GOLDEN[key + "/iterations"][0], e))
    assert stats["iterations"] == GOLDEN[key + "/iterations"][0]
    assert e <= 1e-5
    bits_equal("utm1", utm1.to_numpy(), I["ut"])
    bits_equal("out", out.to_numpy(), ut.to_numpy())


# ---------------------------------------------------------------------------------------------------------------------------------
# uv grids
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.ALL)
def test_reset_uv_grid(hip_backend, name):
    import manta as m
    dims = M.DIMS[name]
    s = _solver(m, dims)
    for oname, off in M.UV_OFFSETS.items():
        uv = _grid(s, m.VecGrid, np.full(M.shape_of(dims) + (3,), np.nan, f32))
        if off is None:
            m.resetUvGrid(uv)
        else:
            m.resetUvGrid(uv, offset=m.vec3(*off))
        check("resetuv/%s/%s" % (name, oname), uv.to_numpy(), M.reset_uv(M.shape_of(dims), off))
        assert f32(m.getUvWeight(uv)) == M.reset_uv(M.shape_of(dims), off)[0, 0, 0, 0]


@pytest.mark.parametrize("case", sorted(M.UVW_GRID_CASES))
def test_update_uv_weight(hip_backend, case):
    import manta as m
    name, oname, n, step, i = M.UVW_GRID_CASES[case]
    s = _solver(m, M.DIMS[name], M.UV_DT)
    s.timeTotal = float(M.uv_time(step))
    uv = _grid(s, m.VecGrid, M.uv_prefill(name))
    off = M.UV_OFFSETS[oname]
    live = s._live
    m.updateUvWeight(resetTime=M.UV_RESET, index=i, numUvs=n, uv=uv, **({} if off is None else {"offset": m.vec3(*off)}))
    assert s._live == live
    model = M.run_uvw_grid(case)
    check("uvwgrid/" + case, uv.to_numpy(), model)
    w = f32(m.getUvWeight(uv))
    assert w.tobytes() == GOLDEN["uvwgrid/%s/weight" % case][0].tobytes() == M.get_uv_weight(model).tobytes()
    assert ("reset" in case) == (not np.array_equal(uv.to_numpy()[0, 1, 1], M.uv_prefill(name)[0, 1, 1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# extrapolateSimpleFlags
# ---------------------------------------------------------------------------------------------------------------------------------
_CLS = {"real": "RealGrid", "int": "IntGrid", "vec": "VecGrid", "flag": "FlagGrid"}


@pytest.mark.parametrize("case", sorted(M.EXTRAP_CASES))
def test_extrapolate_simple_flags(hip_backend, case):
    import manta as m
    name, kind, vtype, dist, ff, ft = M.EXTRAP_CASES[case]
    flags, val, dist, ff, ft = M.extrap_inputs(case)
    s = _solver(m, M.DIMS[name])
    gf, gv = _grid(s, m.FlagGrid, flags), _grid(s, getattr(m, _CLS[vtype]), val)
    _poison_pool(s)
    live = s._live
    m.extrapolateSimpleFlags(flags=gf, val=gv, distance=dist, flagFrom=ff, flagTo=ft)
    assert s._live == live                                  # tmp went back to the pool
    check("extrap/" + case, gv.to_numpy(), M.run_extrap(case))
    bits_equal("flags", gf.to_numpy(), flags)
    if kind == "notarget" and vtype != "int":               # no target cell: no pass writes, whatever val holds
        nan = np.full(val.shape, np.nan, f32)
        gv.from_numpy(nan)
        m.extrapolateSimpleFlags(flags=gf, val=gv, distance=dist, flagFrom=ff, flagTo=ft)
        bits_equal("NaN val", gv.to_numpy(), nan)


def test_extrapolate_defaults_and_mac_grid(hip_backend):
    """the defaults (distance 4, fluid -> obstacle) and a MAC grid, which is a Vec3 grid to the reference's type test"""
    import manta as m
    flags, val, dist, ff, ft = M.extrap_inputs("g33/blob/vec/4")
    s = _solver(m, M.DIMS["g33"])
    gf, gv = _grid(s, m.FlagGrid, flags), _grid(s, m.MACGrid, val)
    m.extrapolateSimpleFlags(gf, gv)
    check("extrap/g33/blob/vec/4", gv.to_numpy(), M.run_extrap("g33/blob/vec/4"))


# ---------------------------------------------------------------------------------------------------------------------------------
# initVortexVelocity
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.VORTEX_CASES))
def test_init_vortex_velocity(hip_backend, name):
    import manta as m
    I = M.vortex_inputs(name)
    s = _solver(m, I["dims"])
    phi, vel = _grid(s, m.RealGrid, I["phiObs"]), _grid(s, m.MACGrid, I["vel"])
    m.initVortexVelocity(phiObs=phi, vel=vel, center=m.vec3(*[float(c) for c in I["center"]]), radius=float(I["radius"]))
    msg = M.same_as_fixture(GOLDEN, "vortex/" + name, vel.to_numpy())
    assert msg is None, msg
    bits_equal("phiObs", phi.to_numpy(), I["phiObs"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the four loops (stated in fields_model.py: the reference's scripts do not travel with the tests) against recorded reference runs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_loop_wave_equation(hip_backend):
    """tools/tests/test_1030_waveeq.py at 23 x 19, 12 steps, implicit from step 6: the mass of every step within 1 ulp, the CG
    iteration count of every implicit step, h and vel within 1e-5 relative"""
    import manta as m
    got = M.wave_loop_pkg(m)
    bits_equal("h0: Box.applyToGrid is the recorder's initial height", got["h0"], GOLDEN["loop/wave/h0"])
    want = GOLDEN["loop/wave/mass"]
    print("mass", got["mass"], "reference", want, "iterations", got["iterations"])
    assert (np.abs(got["mass"].astype(f64) - want.astype(f64)) <= M.ulp(want)).all()
    assert got["iterations"].tolist() == GOLDEN["loop/wave/iterations"].tolist() and (got["iterations"][6:] > 0).all()
    for k in ("h", "vel"):
        e = util.rel_err(got[k], GOLDEN["loop/wave/" + k])
        print(k, "rel. error %.3g" % e)
        assert e <= 1e-5, k


def test_loop_uv_grids(hip_backend):
    """tools/tests/test_1020_uvs.py's main loop at 20 x 30 with 3 uv grids, 20 steps, resetTime 11 (grids 1 and 2 are reset on the
    way): every uv grid and every weight bit for bit"""
    import manta as m
    got = M.uv_loop_pkg(m)
    bits_equal("weights", got["weights"], GOLDEN["loop/uv/weights"])
    for i, uv in enumerate(got["uv"]):
        bits_equal("uv%d" % i, uv, GOLDEN["loop/uv/uv%d" % i])
    start = M.reset_uv(M.shape_of(M.UV_LOOP["dims"]))
    assert all((uv[0, 3:-3, 3:-3] != start[0, 3:-3, 3:-3]).any() for uv in got["uv"])       # the advection moved them


def test_loop_second_order_boundaries(hip_backend):
    """tools/tests/test_1040_secOrderBnd.py at 16 x 16, 10 steps: fractions bit for bit, the CG iteration count of every step, vel
    within 1e-5 relative"""
    import manta as m
    got = M.bnd_loop_pkg(m)
    bits_equal("fractions", got["fractions"], GOLDEN["loop/bnd/fractions"])
    e = util.rel_err(got["vel"], GOLDEN["loop/bnd/vel"])
    print("iterations", got["iterations"], "reference", GOLDEN["loop/bnd/iterations"], "vel rel. error %.3g" % e)
    assert got["iterations"].tolist() == GOLDEN["loop/bnd/iterations"].tolist()
    assert e <= 1e-5


def test_loop_fire(hip_backend):
    """scenes/fire.py's loop at 16^3, 6 steps, adaptive dt, open y bounds, the inflows replaced by copies of seeded fields: dt and CG
    iterations of every step identical, every grid within 1e-5 relative.  The recorder found no cell in this loop in which powf(x, 0.5f)
    differs from sqrtf(x) (loop/fire/powf_cells), so the iteration counts do not rest on that difference staying small."""
    import manta as m
    got = M.fire_loop_pkg(m)
    print("dt", got["dts"], "iterations", got["iterations"], "reference", GOLDEN["loop/fire/iterations"], "powf cells", GOLDEN["loop/fire/powf_cells"])
    bits_equal("dt", got["dts"], GOLDEN["loop/fire/dts"])
    assert got["iterations"].tolist() == GOLDEN["loop/fire/iterations"].tolist()
    for k in M.FIRE_LOOP_GRIDS:
        e = util.rel_err(got[k], GOLDEN["loop/fire/" + k])
        print(k, "rel. error %.3g" % e)
        assert e <= 1e-5, k
    for q, k in enumerate("xyz"):
        e = util.rel_err(got["vel"][..., q], GOLDEN["loop/fire/vel_" + k])
        print("vel", k, "rel. error %.3g" % e)
        assert e <= 1e-5, k
