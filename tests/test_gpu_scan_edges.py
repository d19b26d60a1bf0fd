"""GPU: the sizes at which a prefix sum, a sort or a scratch-block layout of csrc/scan.hip's users can go wrong and which no other
test reaches -- gridParticleIndex with no particle, one particle, every particle in the last cell (the count is the last prefix entry
plus the last counter) and every particle deleted (nothing indexed, every key the tail key n), on 2x2x1 and 3x2x2; adjustNumber with
compress allowed on a system of exactly one particle (the round sorts one pair and scans one element), and a second call that kills
it (the compress plan of an array that becomes empty).  Every case is compared whole and bit for bit with the model the plugin's own
tests use: tests/partls_model.py (particle_index) and tests/nbflip_model.py through the helpers of tests/test_gpu_nbflip.py."""
import numpy as np
import pytest

import nbflip_model as NM
import partls_model as PM
import test_gpu_idp as TI
import test_gpu_nbflip as TN

pytestmark = pytest.mark.gpu

PDELETE = 1 << 10
GPI_DIMS = [(2, 2, 1), (3, 2, 2)]


def gpi_inputs(dims, case):
    """(pos, pflag) of a gridParticleIndex edge case"""
    sx, sy, sz = dims
    last = np.array([sx - 0.5, sy - 0.5, sz - 0.5], np.float32)
    if case == "none":
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
    if case == "one":
        return np.array([[0.25, 1.5, 0.5]], np.float32), np.zeros(1, np.int32)
    if case == "last_cell":
        pos = np.tile(last, (5, 1))
        pos[:, 0] -= np.float32(0.0625) * np.arange(5, dtype=np.float32)      # distinct points of the one cell
        return pos, np.zeros(5, np.int32)
    if case == "all_deleted":
        cells = np.arange(sx * sy * sz)
        pos = np.stack([cells % sx, (cells // sx) % sy, cells // (sx * sy)], axis=1).astype(np.float32) + np.float32(0.5)
        return pos, np.full(len(cells), PDELETE | 1, np.int32)
    raise KeyError(case)


def gpi_expected(dims, case, pos, pflag):
    """the model's answer, and that the inputs take the branch the case is named for"""
    start, cnt, isys = PM.particle_index(dims, pos, pflag)
    n = dims[0] * dims[1] * dims[2]
    if case in ("none", "all_deleted"):
        assert len(isys) == 0 and not cnt.any() and not start.any()
    if case == "one":
        assert len(isys) == 1 and cnt[dims[0]] == 1
    if case == "last_cell":
        assert len(isys) == 5 and cnt[n - 1] == 5 and start[n - 1] == 0 and cnt.sum() == 5
    return start, isys


@pytest.mark.parametrize("case", ["none", "one", "last_cell", "all_deleted"])
@pytest.mark.parametrize("dims", GPI_DIMS, ids=["2x2x1", "3x2x2"])
def test_grid_particle_index_edges(hip_backend, dims, case):
    import manta as m
    pos, pflag = gpi_inputs(dims, case)
    start, isys = gpi_expected(dims, case, pos, pflag)
    s = TI._solver(m, dims)
    pp, _ = TI._parts(m, s, pos, pflag)
    flags, gpi, pindex = s.create(m.FlagGrid), s.create(m.IntGrid), s.create(m.ParticleIndexSystem)
    m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
    assert pindex.np == len(isys)
    assert np.array_equal(gpi.to_numpy().ravel(), start)
    assert np.array_equal(pindex.data[:pindex.np].cpu().numpy(), isys)


# ---- adjustNumber on one particle ------------------------------------------------------------------------------------------------------
ADJUST_DIMS = (2, 2, 1)     # the smallest grid check_dim and nbflip_model.adjust_inputs accept
# the first call keeps the particle (it lies in the liquid, no band) and seeds nothing; the second has a band of half a cell above the
# particle's depth and culls it: with the (0, 0) book the kill is a hit, so the round ends in a compress plan, of one particle, none of
# which stays
ADJUST_CALLS = [((0, 0), dict(minParticles=0, maxParticles=8)), (None, dict(minParticles=0, maxParticles=8, narrowBand=0.5))]


def one_particle_inputs():
    """nbflip_model.adjust_inputs cut down to its first particle, moved to the point of the grid that lies deepest in the liquid"""
    I = NM.adjust_inputs(ADJUST_DIMS, 401, outside=0, deleted_frac=0.0, dense_frac=1.0, max_per_cell=3)
    p = I["parts"]
    assert p.size() >= 1
    p._set_arrays([a[:1].copy() for a in p._arrays()])
    sx, sy, sz = ADJUST_DIMS
    cand = np.array([[i + 0.5, j + 0.5, 0.5] for j in range(sy) for i in range(sx)], np.float32)
    p.pos[0] = cand[np.argmin(NM.interp_real(I["phi"], cand))]
    p.flag[0] = 0
    assert NM.interp_real(I["phi"], p.pos)[0] < -0.75       # in the liquid, and below the second call's band
    p.allow_compress = True
    return I


def one_particle_model(I):
    """the model's states after each call, and that they take the intended branches"""
    p = I["parts"].copy()
    out = []
    for book, kw in ADJUST_CALLS:
        if book is not None:
            p.deletes, p.chunk = book
        p.compresses = 0
        NM.adjust_number(p, I["flags"], I["phi"], segmented=True, exclude=None, **kw)
        q = p.copy()
        q.compresses, q.rounds, q.inserted = p.compresses, p.rounds, p.inserted
        out.append(q)
    kept, gone = out
    assert kept.size() == 1 and kept.compresses == 0 and kept.inserted == 0 and kept.rounds == 1
    assert gone.size() == 0 and gone.compresses == 1 and gone.inserted == 0
    return out


def test_adjust_number_one_particle_kept_then_killed(hip_backend):
    import manta as m
    I = one_particle_inputs()
    want = one_particle_model(I)
    got = TN._run_device(m, I, ADJUST_CALLS, ADJUST_DIMS)
    for ci, (g, w) in enumerate(zip(got, want)):
        TN._compare_state(g, w, "call %d" % ci)
        assert g["stats"]["rounds"] == w.rounds and g["stats"]["inserted"] == 0, g["stats"]
    assert got[0]["stats"]["kills"] == 0 and got[0]["stats"]["compresses"] == 0
    assert got[1]["stats"]["kills"] == 1 and got[1]["stats"]["compresses"] == 1
