"""The z-slab schedule of the multigrid V-cycle (tests/mgslab_model.py: level 0 cut along z, four one-plane exchanges and one
all-gather, the levels >= 1 replicated) against the undivided V-cycle of the numpy model (tests/mg_model.py), bit for bit, on
every level: for 1, 2, 3 and 5 ranks, cuts at even and at odd planes, one-plane slabs (at an odd plane such a slab owns no
coarse plane), an even NZ (whose top coarse plane lies above the last fine plane) and odd ones, and two kinds of system.  The
model poisons every plane a rank does not own with NaN and its ghost planes again before each exchange, so a schedule that
lacked an exchange would not come out equal."""
import functools

import numpy as np
import pytest

import mg_model as M
import mgslab_cases
import mgslab_model as S

SHAPES = [(12, 10, 9), (12, 10, 18), (9, 8, 19)]
# NZ -> the interior boundaries of the ranks' z-ranges
CUTS = {
    9: [(), (4,), (5,), (2, 6), (3, 4), (2, 3, 5, 7)],              # (3, 4): the slab [3, 4) is one odd plane
    18: [(), (9,), (8,), (6, 12), (7, 8), (3, 7, 8, 13), (17,)],     # (7, 8): [7, 8); (17,): the last rank owns plane 17 and coarse plane 9
    19: [(), (9,), (10,), (6, 13), (9, 10), (4, 8, 11, 15), (1, 18)],
}
KINDS = mgslab_cases.KINDS


@functools.lru_cache(maxsize=None)
def system(kind, dims):
    """-> hierarchy, rhs of one of the two kinds of system (mgslab_cases.system)"""
    A, rhs = mgslab_cases.system(kind, dims)
    if kind == "lap":
        return M.setup(dims, A), rhs
    # the level-1 sums of a non-integer system depend on the order of the reference's sorted paths; the schedule does not care
    # which operator level 1 holds, as long as both V-cycles run on the same one: an empty patch takes the model's own sums
    H = M.setup(dims, A, A1_patch=(np.zeros(0, np.int64), np.zeros(0, np.float32)))
    assert H.trivial_found
    return H, rhs


@pytest.mark.parametrize("dims", SHAPES)
def test_shapes_have_two_levels_and_every_world(dims):
    assert len(M.level_sizes(dims)) >= 2
    worlds = sorted(set(len(c) + 1 for c in CUTS[dims[2]]))
    assert worlds == [1, 2, 3, 5]
    one_odd_plane = [c for c in CUTS[dims[2]] for z0, z1 in S.ranges_of(dims[2], c) if z1 - z0 == 1 and z0 % 2 == 1 and z1 < dims[2]]
    assert one_odd_plane, "no cut with a one-plane slab at an odd plane"
    for c in one_odd_plane:
        assert any(S.coarse_planes(z0, z1, dims[2])[0] == S.coarse_planes(z0, z1, dims[2])[1] for z0, z1 in S.ranges_of(dims[2], c))
    cuts = [z for c in CUTS[dims[2]] for z in c]
    assert any(z % 2 == 0 for z in cuts) and any(z % 2 == 1 for z in cuts)


@pytest.mark.parametrize("NZ", [9, 18, 19])
def test_every_coarse_plane_has_one_owner(NZ):
    csz = (NZ + 2) // 2
    for cuts in CUTS[NZ]:
        ranges = S.ranges_of(NZ, cuts)
        owned = [k for z0, z1 in ranges for k in range(*S.coarse_planes(z0, z1, NZ))]
        assert owned == list(range(csz)), (cuts, owned)
        for z0, z1 in ranges:
            for k in range(*S.coarse_planes(z0, z1, NZ)):
                assert z0 <= min(2 * k, NZ - 1) < z1


@functools.lru_cache(maxsize=None)
def undivided(kind, dims):
    H, rhs = system(kind, dims)
    return M.vcycle(H, rhs)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims", SHAPES)
def test_cut_vcycle_equals_undivided(dims, kind):
    H, rhs = system(kind, dims)
    want = undivided(kind, dims)
    assert np.isfinite(want["result"]).all() and np.abs(want["result"]).max() > 0
    for cuts in CUTS[dims[2]]:
        got = S.vcycle(H, rhs, S.ranges_of(dims[2], cuts))
        assert (got["exchanges"], got["gathers"]) == (4, 1)
        assert got["cg_iters"] == want["cg_iters"], cuts
        assert got["result"].tobytes() == want["result"].tobytes(), "result, cuts %r" % (cuts,)
        for l in range(H.nl):
            assert got["x"][l].tobytes() == want["x"][l].tobytes(), "x of level %d, cuts %r" % (l, cuts)
            assert got["b"][l].tobytes() == want["b"][l].tobytes(), "b of level %d, cuts %r" % (l, cuts)


@pytest.mark.parametrize("leave_out", [0, 1, 2, 3])
def test_every_exchange_is_needed(leave_out):
    """with any one of the four exchanges left out (its ghost planes stay poisoned) the result is not the undivided one"""
    dims = (12, 10, 18)
    H, rhs = system("lap", dims)
    want = undivided("lap", dims)
    for cuts in ((9,), (6, 12)):
        got = S.vcycle(H, rhs, S.ranges_of(dims[2], cuts), leave_out=leave_out)
        assert got["exchanges"] == 4 and got["result"].tobytes() != want["result"].tobytes(), (leave_out, cuts)
