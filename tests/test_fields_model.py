"""CPU: the numpy model of the fire, wave-equation and uv-grid plugins (tests/fields_model.py) against the recorded reference
(tests/golden/fields.npz; tools/record_fields.py) for every fixture case -- bit for bit, except `flame` and `heat`, where the reference's
powf(x, 0.5f) may differ from the correctly rounded square root in the last bit: there the model with the recorded differing cells put
in must be the reference's array, and those cells must lie within the bounds of DESIGN.md section 15.  Plus: the literal serial loop of
extrapolateSimpleFlags against the per-pass statement the kernels implement, the branches each fire case exists for, and
updateUvWeight's scalar part across resets."""
import os

import numpy as np
import pytest

import fields_model as M

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fields.npz"))
f32, f64 = np.float32, np.float64


def fixture_is(key, a):
    msg = M.same_as_fixture(GOLDEN, key, a)
    assert msg is None, msg


# ---------------------------------------------------------------------------------------------------------------------------------
# fire
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(M.FIRE_CASES))
def test_fire_model_is_the_reference(case):
    name, absent, par = M.FIRE_CASES[case]
    out, flame = M.run_fire(case)
    assert set(out) == {"fuel", "density", "react"} | (set(M.OPTIONAL) - set(absent))
    for k in out:
        if k != "heat":
            fixture_is("fire/%s/%s" % (case, k), out[k])
    counts = GOLDEN["fire/%s/powf_cells" % case]
    # flame: within 1 ulp of the reference, equal outside the recorded cells
    msg, idx, ref = M.near_fixture(GOLDEN, "fire/%s/flame" % case, flame)
    assert msg is None, msg
    assert idx.size == counts[1] and (np.abs(flame.reshape(-1)[idx].astype(f64) - ref.astype(f64)) <= M.ulp(ref)).all()
    assert (flame.reshape(-1)[idx] != ref).all()
    if "heat" in out:
        msg, idx, ref = M.near_fixture(GOLDEN, "fire/%s/heat" % case, out["heat"])
        assert msg is None, msg
        bound = M.heat_bound(M.fire_flame(case), out["heat"], par["ignitionTemp"], par["maxTemp"]).reshape(-1)[idx]
        assert idx.size == counts[0] and (np.abs(out["heat"].reshape(-1)[idx].astype(f64) - ref.astype(f64)) <= bound).all()
    # border cells of every grid keep the caller's values
    g = M.fire_inputs(name)
    b = ~M.interior_mask(g["fuel"].shape)
    for k in out:
        assert np.array_equal(out[k][b], g[k][b]), k
    assert np.array_equal(flame[b], M.prefill(name, "flame")[b])


def test_powf_differs_somewhere_in_the_fixture():
    """the fixture is large enough to hold cells in which powf(x, 0.5f) is not the correctly rounded square root"""
    total = sum(GOLDEN["fire/%s/powf_cells" % c] for c in M.FIRE_CASES)
    assert total[1] > 0 and total[2] > 20000


def test_fire_branches():
    cnt = {}
    M.run_fire("g33/all", cnt)
    for key in ("fuel_le_eps", "fuel_ge_1", "fuel_clamped", "emit_le_eps", "emit_gt_eps", "density_above_1", "density_below_0",
                "react_zero_heat_kept", "heat_written"):
        assert cnt.get(key, 0) > 0, key
    # density is NOT clamped: the reference drops clamp()'s result.  The fixture itself holds cells above 1.
    out, _ = M.run_fire("g7/all")
    fixture_is("fire/g7/all/density", out["density"])
    I = M.interior(out["density"].shape)
    assert (GOLDEN["fire/g7/all/density"][I] > 1).any()
    assert (np.clip(out["density"], 0, 1) != out["density"])[I].any()
    # react = 0 (burnt out, or -0): flame is +0 and heat keeps the caller's value
    g = M.fire_inputs("g7")
    dead = (out["react"][I] == 0) & (g["fuel"][I] > M.EPS)
    assert dead.any() and np.array_equal(out["heat"][I][dead], g["heat"][I][dead])
    assert not np.signbit(M.pow_half(np.array([-0.0], f32)))[0] and M.pow_half(np.array([-np.inf], f32))[0] == np.inf
    assert np.isnan(M.pow_half(np.array([-1.0], f32)))[0]
    # the single interior cell of the 3 x 3 grid burns, emits and ends above 1
    out3, _ = M.run_fire("g3/all")
    assert out3["density"][0, 1, 1] > 1 and out3["heat"][0, 1, 1] != M.fire_inputs("g3")["heat"][0, 1, 1]


def test_each_optional_grid_absent():
    full, _ = M.run_fire("g7/all")
    for k in M.OPTIONAL:
        cnt = {}
        out, _ = M.run_fire("g7/no_" + k, cnt)
        assert k not in out and cnt["absent_" + k] == 1 and sum(cnt["absent_" + o] for o in M.OPTIONAL) == 1
        for o in out:           # the other grids do not depend on the absent one
            assert np.array_equal(out[o].view(np.uint32), full[o].view(np.uint32)), (k, o)
    cnt = {}
    out, _ = M.run_fire("g7/none", cnt)
    assert set(out) == {"fuel", "density", "react"} and all(cnt["absent_" + o] == 1 for o in M.OPTIONAL)


# ---------------------------------------------------------------------------------------------------------------------------------
# wave equation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.ALL)
def test_wave_model_is_the_reference(name):
    v = M.secderiv_input(name)
    fixture_is("secderiv/" + name, M.sec_deriv_2d(v, M.prefill(name, "curv")))
    for kind in M.SUM_KINDS:
        h = M.sum_input(name, kind)
        fixture_is("sum/%s/%s/sum" % (name, kind), np.array([M.total_sum(h)], f32))
        fixture_is("sum/%s/%s/grid" % (name, kind), M.normalize_sum_to(h, M.SUM_TARGET))
    for cn in (0, 1):
        model = M.run_wave_system(name, bool(cn))
        for k, a in model.items():
            fixture_is("wavesys/%s/%d/%s" % (name, cn, k), a)
        assert not model["rhs"][~M.interior_mask(model["rhs"].shape)].any()
    a, b = M.run_wave_system(name, False), M.run_wave_system(name, True)
    assert name == "g3" or (a["rhs"] != b["rhs"]).any()
    assert all(np.array_equal(a[k], b[k]) for k in ("A0", "Ai", "Aj", "Ak"))


def test_exact_sums_do_not_depend_on_the_order():
    for name in M.ALL:
        h = M.sum_input(name, "exact")
        x = h[M.interior(h.shape)].astype(f64).ravel()
        assert M.total_sum64(h) == x[::-1].sum() == np.sum(x) and np.abs(x).max() <= 4 and ((x * 64) == np.round(x * 64)).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# uv grids
# ---------------------------------------------------------------------------------------------------------------------------------
def test_uv_model_is_the_reference():
    for name in M.ALL:
        for oname, off in M.UV_OFFSETS.items():
            fixture_is("resetuv/%s/%s" % (name, oname), M.reset_uv(M.shape_of(M.DIMS[name]), off))
    cnt = {}
    got = [M.uv_weight(M.uv_time(step), M.UV_DT, M.UV_RESET, i, n, cnt) for n, step, i in M.UVW_SCALARS]
    fixture_is("uvw/weights", np.array([w for w, _ in got], f32))
    fixture_is("uvw/resets", np.array([r for _, r in got], np.int32))
    for key in ("total_le_eps", "reset", "ramp_down"):
        assert cnt.get(key, 0) > 0, key
    for case in M.UVW_GRID_CASES:
        uv = M.run_uvw_grid(case)
        fixture_is("uvwgrid/" + case, uv)
        fixture_is("uvwgrid/%s/weight" % case, np.array([M.get_uv_weight(uv)], f32))
        assert not uv[0, 0, 0, 1:].any()


def test_update_uv_weight_across_a_reset():
    """numUvs 1, 2, 3: every grid resets exactly when its normalised time wraps, the weights of one step sum to 1 (or are all 1 in the
    uvWTotal <= 1e-6 branch), and the package's host half is the model's"""
    import manta  # noqa: F401
    from mantaflow_amd import plugins
    for n in (1, 2, 3):
        nresets = 0
        for step in range(25):
            t = M.uv_time(step)
            ws = []
            for i in range(n):
                w, reset = M.uv_weight(t, M.UV_DT, M.UV_RESET, i, n)
                pw, preset = plugins._uv_weight_scalars(float(t), M.UV_DT, M.UV_RESET, i, n)
                assert f32(pw).tobytes() == w.tobytes() and preset == reset
                ws.append(w)
                nresets += reset
                now = (f64(t) + i * M.UV_RESET / n) / M.UV_RESET
                assert reset == (step > 0 and int(np.floor(now + 1e-9)) > int(np.floor(now - M.UV_DT / M.UV_RESET + 1e-9)))
            if n == 1 and step == 0:
                assert ws == [f32(1)]                                # the <= 1e-6 branch sets both to 1
            elif n > 1:
                assert abs(sum(f64(w) for w in ws) - 1) < 1e-6
        assert nresets >= n
    cnt = {}
    assert M.uv_weight(0.0, 0.5, 11.0, 0, 1, cnt) == (f32(1), False) and cnt["total_le_eps"] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# extrapolateSimpleFlags
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(M.EXTRAP_CASES))
def test_extrapolate_model_is_the_reference(case):
    fixture_is("extrap/" + case, M.run_extrap(case))


def test_extrapolate_cases_cover_their_conditions():
    cnt = {}
    flags, val, dist, ff, ft = M.extrap_inputs("g33/blob/real/6")
    out = M.extrapolate(flags, val, dist, ff, ft, cnt)
    assert all(cnt["written_pass_%d" % d] > 0 for d in range(1, 7))
    deep = M.extrapolate(flags, val, 7, ff, ft)
    assert (deep != out).any()                                  # distance 6 stops short of the block's core
    for case in ("g7/notarget/real/4", "g2d/notarget/vec/4"):
        flags, val, dist, ff, ft = M.extrap_inputs(case)
        assert not (flags & ft).any() and np.array_equal(M.run_extrap(case), val)
        val[...] = np.nan                                       # no pass writes, whatever val holds
        assert np.isnan(M.extrapolate(flags, val, dist, ff, ft)).all()
    cnt = {}
    M.run_extrap("g6/both/real/4", cnt)
    assert cnt["both_flags"] > 0
    flags, val, dist, ff, ft = M.extrap_inputs("g33/scene/flag/2")
    assert val.dtype == np.int32 and (ff, ft, dist) == (M.TypeObstacle, M.TypeFluid, 2)
    neg = M.extrap_val("g33", "int")
    assert (neg < 0).any()                                      # the truncating division is exercised on negative sums


def test_serial_loop_equals_the_per_pass_statement():
    """the reference's loop is serial and in place; within pass d it reads only cells with tmp == d and writes only cells that become
    d + 1, so it computes what one launch per pass computes: 1000 random small cases, all value types, 2-D
    and 3-D, three flag pairs, cells with both flags, distances 0..5"""
    kinds = set()
    for seed in range(1000):
        flags, val, dist, ff, ft = M.random_extrap_case(seed)
        a, b = M.extrapolate_serial(flags, val, dist, ff, ft), M.extrapolate(flags, val, dist, ff, ft)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), seed
        if (a != val).any():
            kinds.add((val.dtype.name, val.ndim, flags.shape[0] == 1))
    assert len(kinds) >= 5
