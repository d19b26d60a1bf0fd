"""CPU: the numpy model of the vortex particle family (tests/vortex_model.py) against the reference's recorded outputs
(tests/golden/vortex.npz, tools/record_vortex.py), and the condition each case exists for, from the model's counters."""
import os

import numpy as np
import pytest

import vortex_model as M

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vortex.npz"))
_counters = {}


@pytest.mark.parametrize("name", list(M.CASES))
def test_velocity_and_the_three_modes_are_the_reference(name):
    cnt = _counters.setdefault(name, {})
    assert M.same_as_fixture(GOLDEN, "vel/%s/u" % name, M.case_velocity(name, cnt)) is None
    for mode in M.MODES:
        assert M.same_as_fixture(GOLDEN, "end/%s/%d" % (name, mode), M.run_case(name, mode)) is None, mode


def _cnt(name):
    if name not in _counters:
        M.case_velocity(name, _counters.setdefault(name, {}))
    return _counters[name]


def test_each_case_meets_its_condition():
    e = _cnt("edge")
    for key in ("at_cutoff_kept", "ulp_beyond_cutoff", "rho2_small", "branch_zero", "branch_unit", "branch_scaled", "sigma_zero", "deleted_sources",
                "zeroed_targets"):
        assert e.get(key, 0) > 0, key
    assert e["coincident"] > 14                                 # more than every particle's term on itself
    assert _cnt("underflow")["underflow"] > 0 and _cnt("underflow")["inside"] > 0
    assert _cnt("self257")["deleted_sources"] > 0 and _cnt("self257")["zeroed_targets"] > 0
    assert _cnt("mesh1000_600")["zeroed_targets"] > 0 and _cnt("mesh1000_600")["deleted_sources"] > 0      # fixed nodes
    for name, (kind, nT, nS, *_rest) in M.CASES.items():
        if nT > 1 and nS > 1:
            c = _cnt(name)
            assert 0 < c["inside"] < c["pairs"], name             # the cutoff removes some pairs and keeps some
    # the sizes around the workgroup (64 targets) and the tile (256 sources)
    assert {c[1] for c in M.CASES.values()} >= {0, 1, 63, 64, 65, 257, 1000} and {c[2] for c in M.CASES.values()} >= {0, 1, 255, 256, 257, 600}
    # the cutoff pair really is exact: r = (1, 1, 2), sigma = 1
    P = M._edge_particles()
    r = P["pos"][1] - P["pos"][0]
    assert np.float32(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) == np.float32(6) and P["sigma"][0] == 1
    u = M.case_velocity("edge")
    assert u[1].any() and not u[12].any()                        # the kept pair moves its target; the deleted particle has u = 0


def test_unknown_mode_raises():
    with pytest.raises(RuntimeError, match="unknown integration type"):
        M.run_case("self1", 3)


def test_seeding_is_the_reference():
    cnt = {}
    res = M.run_seed_cases(cnt)
    for name in M.SEED_ORDER:
        arrays, start, end = res[name]
        for ch in M.CHANNELS:
            assert M.same_as_fixture(GOLDEN, "seed/%s/%s" % (name, ch), arrays[ch]) is None, (name, ch)
        assert [start, end] == GOLDEN["seed/%s/cursors" % name].tolist()
    c = cnt
    assert 0 < c["box3"]["seeded"] < c["box3"]["cells"]                                  # probability * dt in between
    assert c["above1"]["seeded"] == c["above1"]["cells"] > 0                             # above 1
    assert c["zero"].get("seeded", 0) == 0 and c["zero"]["rejected"] == c["zero"]["cells"] > 0
    assert res["zero"][2] - res["zero"][1] == c["zero"]["cells"]                         # one draw per cell
    assert res["above1"][2] - res["above1"][1] == 8 * c["above1"]["cells"]               # and seven more per particle
    assert len(M.SEED_CASES["twice"][2]) == 2 and res["twice"][1] == res["zero"][2]      # the stream continues
    assert res["box2"][0]["pos"].shape[0] > 0 and (res["box2"][0]["pos"][:, 2] < 1).all() and res["box2"][0]["pos"][:, 2].any()     # z still drawn
    assert res[M.SEED_ORDER[0]][1] == 0
    # a reset: a fresh stream reproduces the first case
    st, P = M.Stream(), M.new_system()
    dims, dt, calls = M.SEED_CASES["box3"]
    M.seed_k41(P, st, dims, dt, calls[0][0], *calls[0][1:])
    assert M.same_as_fixture(GOLDEN, "seed/box3/pos", M.system_arrays(P)["pos"]) is None


@pytest.mark.parametrize("name", list(M.DENSITY_CASES))
def test_density_from_levelset_is_the_reference(name):
    phi, value, sigma = M.density_inputs(name)
    cnt = {}
    assert M.same_as_fixture(GOLDEN, "density/%s" % name, M.density_from_levelset(phi, value, sigma, cnt)) is None
    if name == "d2":
        assert cnt["border"] == phi.size                         # k < 2 on a 2-D grid: everything is border
    else:
        assert min(cnt["border"], cnt["below"], cnt["above"], cnt["ramp"]) > 0
        assert (phi == sigma).any() and (phi == -sigma).any()


def test_mark_as_fixed_is_the_reference():
    pos, flags = M.fixed_inputs()
    for ex in (0, 1):
        got = M.mark_as_fixed(pos, flags, M.FIXED_BOX, bool(ex))
        assert np.array_equal(got, GOLDEN["fixed/%d" % ex])
    a, b = GOLDEN["fixed/0"], GOLDEN["fixed/1"]
    assert (a != b).any() and ((flags & 1) != (b & 1)).any() and ((b & ~1) == (flags & ~1)).all()
