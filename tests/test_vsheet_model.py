"""CPU: the numpy model of the vortex-sheet stages (tests/vsheet_model.py) against the recorded reference (tests/golden/vsheet.npz; how
each array was produced: tools/record_vsheet.py).  Every arithmetic stage is bit for bit; the smoothing weights -- the one transcendental,
float exp in the reference against the fp64 exp rounded once -- are within vsheet_model.WEIGHT_ULPS, and the passes
are bit for bit from the recorded table.  The quirks are asserted on the reference's own arrays."""
import numpy as np
import pytest

import mesh_model as MM
import meshops_model as MO
import vsheet_model as M

f32 = np.float32
G = M.golden()


def _same(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, got.dtype, want.shape, want.dtype)
    assert got.tobytes() == want.tobytes(), "%s: %d of %d words differ" % (tag, int((got.view("u4") != want.view("u4")).sum()), got.size)


def test_defaults_after_a_rebuild_are_the_reference_s():
    for k, v in M.DEFAULTS.items():
        assert (G["defaults/" + k] == f32(v)).all() and G["defaults/" + k].shape[0] == 4, k
        assert (M.default_sheet(4)[k] == G["defaults/" + k]).all()
    assert not G["defaults/tex1"].any() and not G["defaults/turb"].any()


@pytest.mark.parametrize("name", sorted(M.MESHES))
def test_calc_smoke_and_source(name):
    m = M.with_fixed(M.MESHES[name](), name)
    st = M.sheet_state(name, m["tris"].shape[0])
    v, smoke = M.calc_vorticity(m, st["circulation"])
    _same("calc/vorticity", v, G["calc/%s/vorticity" % name])
    _same("calc/smokeAmount", smoke, G["calc/%s/smokeAmount" % name])
    for sname, shape in M.SMOKE_SHAPES.items():
        _same("smoke/" + sname, M.smoke_inflow(m, shape, 0.37, st["smokeAmount"]), G["smoke/%s/%s" % (name, sname)])
    vel, old = M.mac_grid("src-" + name), M.mac_grid("src-old-" + name)
    for vname, (with_vel, maxAmount, mult, scale) in M.SOURCE_VARIANTS.items():
        w, _ = M.vorticity_source(m, st["vorticity"], M.GRAVITY, M.DIMS, M.DT, vel if with_vel else None, old if with_vel else None, scale, maxAmount, mult)
        _same("source/" + vname, w, G["source/%s/%s" % (name, vname)])


def test_calc_vorticity_quirks_on_the_reference_s_arrays():
    """smokeAmount = 0 in both branches; zero vorticity below the area threshold, which compares in double"""
    m = M.MESHES["degenerate"]()
    small = M.face_area(m).astype(np.float64) < 1e-10
    assert 0 < small.sum() < small.size
    ref = G["calc/degenerate/vorticity"]
    assert not ref[small].any() and ref[~small].any(1).all()
    assert not G["calc/degenerate/smokeAmount"].any() and not G["calc/sphere17/smokeAmount"].any()
    assert (M.sheet_state("degenerate", small.size)["smokeAmount"] != 0).all()          # it was not zero before


def test_source_clamps_with_the_norm_taken_after_the_update():
    name = "sphere17"
    m = M.with_fixed(M.MESHES[name](), name)
    st = M.sheet_state(name, m["tris"].shape[0])
    _, maxAmount, mult, scale = M.SOURCE_VARIANTS["clamped"]
    ref = G["source/%s/clamped" % name]
    w, v = M.vorticity_source(m, st["vorticity"], M.GRAVITY, M.DIMS, M.DT, M.mac_grid("src-" + name), M.mac_grid("src-old-" + name), scale, maxAmount, mult)
    hit = v > f32(maxAmount)
    before = M.norm3(st["vorticity"]) > f32(maxAmount)
    assert hit.any() and (~hit).any() and (hit != before).any()          # a clamp decided on the old norm would pick other triangles
    assert (M.norm3(ref)[hit] <= f32(maxAmount) * f32(1 + 1e-6)).all() and (M.norm3(ref)[~hit] <= f32(maxAmount)).all()
    # fixed triangles get no source: only `*= mult`
    fixed = M.tri_fixed(m) & ~hit
    assert fixed.any()
    _same("fixed", ref[fixed], (st["vorticity"] * f32(mult))[fixed])


@pytest.mark.parametrize("name", sorted(M.MESHES) + sorted(M.OPEN_MESHES))
def test_smoothing_weights_within_the_bound_and_passes_bit_for_bit(name):
    m = (M.MESHES.get(name) or M.OPEN_MESHES[name])()
    T = m["tris"].shape[0]
    opp = MO.corners(m["tris"])[0]
    st = M.sheet_state(name, T)
    for sigma in M.SMOOTH_SIGMAS:
        key = "smooth/%s/%g" % (name, sigma)
        w_ref, idx_ref = G[key + "/weights"], G[key + "/index"]
        arg, _, has = M.smooth_args(m, opp, sigma)
        assert M.weights_decided(arg[has]) == 0
        w, idx = M.smooth_weights(m, opp, sigma)
        assert np.array_equal(idx, idx_ref)
        assert M.ulps_apart(w, w_ref).max(initial=0) <= M.WEIGHT_ULPS
        assert not w[~has].any() and not idx[~has].any() and not w_ref[~has].any()
        for it in M.SMOOTH_ITERS:
            _same("%s/out%d" % (key, it), M.smooth_iterate(w_ref, idx_ref, st["vorticity"], it, M.ALPHA)[1], G["%s/out%d" % (key, it)])


def test_smoothing_reads_the_weight_at_the_neighbour_triangle_s_number():
    """vortexplugins.cpp:158 is weights[index[idx]], not weights[idx]: the reference's output is the former's"""
    name, sigma = "sphere17", 0.7
    key = "smooth/%s/%g" % (name, sigma)
    st = M.sheet_state(name, G[key + "/index"].shape[0] // 3)
    by_corner = M.smooth_iterate_by_corner(G[key + "/weights"], G[key + "/index"], st["vorticity"], 3, M.ALPHA)
    assert by_corner.tobytes() != G[key + "/out3"].tobytes()
    assert (np.abs(by_corner - G[key + "/out3"]) > 1e-3).any()
    assert int(G["smooth/weight_stats"][2]) <= M.WEIGHT_ULPS


def test_texcoord_inflow_calls_of_one_process():
    m = M.MESHES[M.INFLOW_MESH]()
    n = m["pos"].shape[0]
    t0, tex1, tex2 = np.zeros(3, f32), np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    for q, shape in enumerate(M.INFLOW_CALLS):
        t0, tex1, tex2 = M.texcoord_inflow(M.DIMS, M.mac_grid("inflow%d" % q), shape, M.DT, t0, m["pos"], tex1, tex2)
        _same("t0", t0, G["inflow/%d/t0" % q])
        _same("tex1", tex1, G["inflow/%d/tex1" % q])
        _same("tex2", tex2, G["inflow/%d/tex2" % q])
        if q == 1:
            tex1 = tex2 = M.reinit_tex(m["pos"], t0)
            _same("reinit", tex1, G["inflow/reinit"])
    # the offset is carried from call to call, and a shape without a cell gives NaN (0 / 0), for good
    assert G["inflow/0/t0"].tobytes() != G["inflow/2/t0"].tobytes()
    assert len(M.inflow_cells(M.DIMS, M.INFLOW_CALLS[3])) == 0 and np.isnan(G["inflow/3/t0"]).all()
    assert not np.isnan(G["inflow/2/t0"]).any()


def test_recorded_loop_stage_by_stage():
    C = M.LOOP
    m, flags = M.loop_inputs()
    opp = MO.corners(m["tris"])[0]
    dims, dt = C["dims"], C["dt"]
    pos, st = m["pos"].copy(), M.default_sheet(m["tris"].shape[0])
    for step in range(C["steps"]):
        cur = dict(m, pos=pos)
        vel, old = M.loop_velocities(step)
        st["smokeAmount"] = M.smoke_inflow(cur, C["smoke"], C["amount"], st["smokeAmount"])
        st["vorticity"], _ = M.vorticity_source(cur, st["vorticity"], C["gravity"], dims, dt, vel, old, C["scale"], C["maxAmount"], C["mult"])
        w_ref = G["loop/%d/weights" % step]
        w, idx = M.smooth_weights(cur, opp, C["sigma"])
        assert M.ulps_apart(w, w_ref).max() <= M.WEIGHT_ULPS
        st["vorticitySmoothed"] = M.smooth_iterate(w_ref, idx, st["vorticity"], C["iters"], C["alpha"])[1]
        mvort, _, vbound = M.spread(cur, st["vorticity"], flags, dims, C["vic_sigma"], want_bound=True)
        assert (np.abs(G["loop/%d/vic_vort" % step].T.astype(np.float64) - mvort).max(1) <= vbound).all()
        pos = np.ascontiguousarray(MM.advect_nodes(dims, G["loop/%d/vic_vel" % step], np.ascontiguousarray(pos.T), m["flags"], dt, 2).T)
        for k in ("vorticity", "vorticitySmoothed", "smokeAmount"):
            _same("loop/%d/%s" % (step, k), st[k], G["loop/%d/%s" % (step, k)])
        _same("loop/%d/pos" % step, pos, G["loop/%d/pos" % step])
        _same("loop/%d/tex1" % step, M.reinit_tex(pos, (0, 0, 0)), G["loop/%d/tex1" % step])
    assert 0 < (st["smokeAmount"] == f32(C["amount"])).sum() < st["smokeAmount"].size


@pytest.mark.parametrize("name", sorted(M.vic_cases()))
def test_spreading_within_the_derived_bound_of_the_reference(name):
    dims, sigma, T, rev = M.vic_cases()[name]
    m, vorticity = M.vic_soup(dims, T, 1, rev)
    flags = M.vic_flags(dims)
    model, wnorm, bound = M.spread(m, vorticity, flags, dims, sigma, want_bound=True)
    ref = np.ascontiguousarray(G["vic/%s/vort" % name].T)
    err = np.abs(ref.astype(np.float64) - model).max(1)
    assert (err <= bound).all()
    assert not ref[bound == 0].any() and not model[bound == 0].any()          # where nothing lands the entry is exactly 0
    hit = bound > 0
    print("%s: largest error %.3g of the bound, %d of %d entries not bit-identical" % (
        name, float((err[hit] / bound[hit]).max()) if hit.any() else 0.0, int((ref != model).any(1).sum()), int(hit.sum())))
    if T >= 200:
        assert np.isinf(wnorm).any() or dims[0] < 20 and sigma >= 2        # a triangle whose whole stencil is non-fluid: sum == 0
        assert (M.face_area(m) == 0).any()
    if name.endswith("_rev"):                     # the merge order shows: the other numbering gives other bits somewhere
        fwd = M.spread(*M.vic_soup(dims, T, 1, False), flags, dims, sigma)[0]
        assert fwd.tobytes() != model.tobytes() and np.allclose(fwd, model, rtol=1e-4, atol=1e-5)


def test_spreading_is_decided_under_a_last_bit_perturbation_of_cos():
    for name in ("g7_s2.5_t257", "g7_s1.5_t65"):
        dims, sigma, T, rev = M.vic_cases()[name]
        assert not M.spread_undecided(M.vic_soup(dims, T, 1, rev)[0], M.vic_flags(dims), dims, sigma), name


def test_precondition_0_and_3_are_the_reference_s_assertion():
    for bad in (0, 3):
        assert bytes(G["vic/precondition%d" % bad]).decode() == "GridCg<APPLYMAT>::setICPreconditioner: Invalid method specified."
    for name in M.VIC_SOLVES:
        for kind in ("mac", "vec3"):
            assert G["vic/%s/%s/iterations" % (name, kind)].shape == (3,)
