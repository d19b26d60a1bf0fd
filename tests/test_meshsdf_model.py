"""CPU: the numpy model of mesh level sets (tests/meshsdf_model.py) against the recorded reference (tests/golden/meshsdf.npz; how it was
produced: tools/record_meshsdf.py), and the model's own statements against each other.

Model vs reference, per case: the conditions that go with the tolerance are asserted first from the model's pre-flood field -- no value
of a written cell within its bound of cutoff - 1 or of 0 (cells whose every n.r is zero are exact zeros and exempt).  Then the
reference's field, rebuilt from the fixture and proven by its SHA-256, differs from the model's only in written, unflooded cells and
there by at most (2 * 2^-23 + 4 n 2^-24) A / S + 2^-23 |phi_ref| (glibc's expf against the fp64 exp rounded once);
the flooded set, the written set and every sign are the reference's exactly.  The number of cells not bit-identical is printed, not
capped (the recording: 0 to 16 per case, 89 of 29 667 for 5000 random triangles).

sc_1_7_* have cutoff / sigma = 7: the issue's grid of sigma and cutoff values names that combination; its smallest weight is exp(-49),
far above the subnormal range (which begins to matter near 9.3)."""
import numpy as np
import pytest

import meshsdf_model as M

GOLDEN = np.load(M.GOLDEN)
f32 = np.float32


@pytest.mark.parametrize("name", M.CASES)
def test_model_equals_the_recorded_reference_within_the_bound(name):
    R = M.model(name)
    assert M.margin_ok(R), "a pre-flood value of the model lies within its bound of cutoff - 1 or of 0"
    ref = M.reference_phi(GOLDEN, name)
    model, cut = R["phi"], R["P"]["cutoff"]
    d = np.nonzero(ref.view(np.uint32) != model.view(np.uint32))[0]
    print("%s: %d of %d written cells not bit-identical to the reference" % (name, d.size, int(R["C"]["written"].sum())))
    assert d.size == int(GOLDEN[name + "/ndiff"][0])
    flooded = R["phi"].view(np.uint32) != R["pre"].view(np.uint32)
    assert R["C"]["written"][d].all() and not flooded[d].any()
    assert (np.abs(ref[d].astype(np.float64) - model[d]) <= M.bound(R["C"], ref)[d]).all()
    assert np.array_equal(ref == cut, model == cut) and np.array_equal(ref < 0, model < 0)
    unwritten = ~R["C"]["written"]
    assert np.isin(ref[unwritten], (cut, -cut)).all()


def test_the_cases_meet_the_conditions_they_exist_for():
    cnt = {n: M.model(n)["counters"] for n in M.CASES}
    assert cnt["empty"]["sources"] == 0 and (M.model("empty")["phi"] == -4.0).all() and cnt["empty"]["flooded"] == 0
    assert cnt["outside"]["binned"] == 0 and (M.model("outside")["phi"] == -4.0).all()
    assert cnt["faces"]["dropped"] == 5 and cnt["faces"]["binned"] == 5
    cells = M.cell_index(M.model("faces")["spos"], M.case("faces")["dims"])
    assert cells[:4].tolist() == [0 + 12 * (3 + 11 * 3), 3 + 12 * (0 + 11 * 3), 3 + 12 * (3 + 11 * 0), 0]      # (-1, 0) lands in cell 0
    assert (cells[4:7] == -1).all() and cells[7] == 11 + 12 * (10 + 11 * 9) and (cells[8:] == -1).all()
    assert cnt["zero_area"]["norm_zero"] == 2
    for k, big in M.BIG_EXPECT.items():
        for sfx in "sl":
            plan = M.tri_plan(M.case(k + sfx)["pos"])
            assert plan[0] == big and (plan[1] == 0 or plan[2] == 0 or big == 7), (k, sfx, plan)
    assert cnt["big7l"]["skipped_w"] > 0 and cnt["big7l"]["sources"] > 1
    assert min(M.model("span")["per_tri"]) > 2000 and cnt["span"]["skipped_w"] > 2000
    assert cnt["dense"]["max_in_cell"] >= 200
    assert [M.case("rand%d" % n)["tris"].shape[0] for n in (1, 63, 64, 65, 5000)] == [1, 63, 64, 65, 5000]
    assert cnt["rand5000"]["dropped"] > 0
    assert M.case("mult")["mesh_gs"] != M.case("mult")["dims"]
    inside = lambda n: M.model(n)["phi"].reshape(28, 28, 28)[14, 14, 14]
    assert inside("sphere_closed") == -2.0 and inside("sphere_open") == 2.0
    for n in M.SC_CASES:
        R, dims = M.model(n)["P"]["intRadius"], M.case(n)["dims"]
        if n.endswith("_7_754"):
            assert R >= max(dims) - 1                                  # every cell's block is clamped on every side


def test_stack_loop_equals_closure_on_1000_random_small_grids():
    seen_flood = 0
    for q in range(1000):
        dims, v, cutoff = M.flood_field("rand%d" % q)
        a, steps = M.flood_closure(v, dims, cutoff)
        b = M.flood_stack(v, dims, cutoff)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (q, dims, cutoff)
        seen_flood += steps > 1
    assert seen_flood > 100


@pytest.mark.parametrize("name", ["snake", "corner"] + ["rand%d" % q for q in range(0, 1000, 50)])
def test_tile_rounds_end_in_the_closure(name):
    dims, v, cutoff = M.flood_field(name)
    a, rounds = M.tile_rounds(v, dims, cutoff)
    assert np.array_equal(a.view(np.uint32), M.flood_closure(v, dims, cutoff)[0].view(np.uint32))
    if name == "snake":
        assert rounds - 1 > 1          # the channel crosses tile boundaries back and forth
        assert (a.reshape(dims[::-1])[5, 2:18, 16] == cutoff).all()
    if name == "corner":
        f = a.reshape(dims[::-1])
        assert (f[9:11, 7:12, 8:14] == -1.0).all() and f[16, 19, 23] == cutoff


def test_host_scalars():
    P = M.params(2., -1.)
    assert (P["cutoff"], P["intRadius"], P["cutoff2"], P["isigma2"]) == (4.0, 4, 16.0, 0.25)
    assert P["safeRadius2"] == f32(f32(4.0 + np.sqrt(3.0) * 0.5) ** 2)
    assert M.params(2.5, 7.)["intRadius"] == 7 and M.params(1., 3.)["intRadius"] == 3 and M.params(1., 2.5)["intRadius"] == 3


def test_elementwise_statements():
    sdf = np.array([-1, 0, 1, -0.5, np.nan, -2], f32)
    flags = np.array([1, 1, 1, 2, 1, 4], np.int32)
    g = np.arange(6, dtype=f32)
    assert M.apply_mesh_to_grid(g, sdf, f32(9)).tolist() == [9, 1, 2, 9, 4, 9]
    assert M.apply_mesh_to_grid(g, sdf, f32(9), flags).tolist() == [9, 1, 2, 3, 4, 9]
    v = np.zeros((3, 6), f32)
    assert M.apply_mesh_to_grid(v, sdf, (1, 2, 3), flags)[:, 0].tolist() == [1, 2, 3]
    assert M.apply_density(flags, g, sdf, 7, 0.).tolist() == [7, 7, 2, 3, 7, 5]
    for q in range(len(M.INFLOW_ARGS)):
        assert np.array_equal(M.sha(M.inflow_model(M.INFLOW_CASE, q)), GOLDEN["inflow/%d/sha" % q])       # the recorded densityInflowMesh
