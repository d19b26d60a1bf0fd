"""GPU: averagedParticleLevelset / improvedParticleLevelset through the package on the HIP backend, against the reference fixture
tests/golden/partls.npz (how each array was produced: tests/test_partls_model.py), against the numpy model on seeded random inputs,
and a FLIP loop against a recorded reference run.

averagedParticleLevelset is compared bit for bit.  improvedParticleLevelset calls the device's fp64 pow / acos / cos / sin, which need
not round like the C library's; each result is rounded to fp32 at once, so a difference needs the fp64 value within about 1e-16
(relative) of an fp32 rounding boundary.  The rule, per case:

  * with smoothen = smoothenNeg = 0 at most one corrected cell may differ from the reference, by no more than
    rAcc * 3 / (t_high - t_low) * 4 * 2^-23 * max(1, |maxEV|) + 2^-23 * |phi_ref|      (partls_model.stage_bound);
  * with smoothing the result is bit-identical, except within smoothen + smoothenNeg cells (Manhattan distance) of such a cell.

Every test prints the number of differing cells it saw.  Measured on an MI355X: 0 in every case (README, "Averaged and improved
particle level sets")."""
import os
import zlib

import numpy as np
import pytest

import partls_model as M
import util

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partls.npz"))


def _solver(m, dims):
    return m.Solver(name="t", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)


class Scene(object):
    """particles, their index and a garbage-filled phi on one solver"""

    def __init__(self, m, dims, I, solver=None):
        self.m, self.dims = m, dims
        s = self.s = solver or _solver(m, dims)
        self.pp = s.create(m.BasicParticleSystem)
        self.pp.set_positions(I["pos"], I["pflag"])
        self.pt = None
        if I.get("ptype") is not None:
            self.pt = self.pp.create(m.PdataInt)
            self.pt.from_numpy(I["ptype"])
        self.exclude = I.get("exclude", 0)
        self.flags, self.gpi, self.pindex, self.phi = s.create(m.FlagGrid), s.create(m.IntGrid), s.create(m.ParticleIndexSystem), s.create(m.LevelsetGrid)
        m.gridParticleIndex(parts=self.pp, flags=self.flags, indexSys=self.pindex, index=self.gpi)

    def run(self, improved, **kw):
        m = self.m
        garbage = np.random.RandomState(7).uniform(-1e6, 1e6, self.dims[::-1]).astype(np.float32)
        garbage.ravel()[::5] = np.nan
        self.phi.from_numpy(garbage)            # overwritten everywhere
        fn = m.improvedParticleLevelset if improved else m.averagedParticleLevelset
        fn(self.pp, self.pindex, self.flags, self.gpi, self.phi, ptype=self.pt, exclude=self.exclude, **kw)
        return self.phi.to_numpy()


def _differ(a, b):
    return np.argwhere(np.ascontiguousarray(a, np.float32).view(np.uint32) != np.ascontiguousarray(b, np.float32).view(np.uint32))


def check_improved(tag, got_stage, ref_stage, got_phi, ref_phi, pAcc, rAcc, kw):
    """the rule of the module docstring; returns the number of differing stage cells"""
    d = _differ(got_stage, ref_stage)
    print("%s: %d differing cell(s) before smoothing" % (tag, len(d)), [tuple(c) for c in d])
    assert len(d) <= 1, (tag, d)
    for c in d:
        k, j, i = (int(v) for v in c)
        sz, sy, sx = ref_stage.shape
        interior = 0 < i < sx - 1 and 0 < j < sy - 1 and (sz == 1 or 0 < k < sz - 1)
        assert interior and rAcc[k, j, i] > M.EPS, (tag, "a cell that is not corrected differs", c)
        bound = M.stage_bound(pAcc, rAcc, (k, j, i), kw.get("t_low", 0.4), kw.get("t_high", 3.5), ref_stage[k, j, i])
        delta = abs(float(got_stage[k, j, i]) - float(ref_stage[k, j, i]))
        print("%s: cell %s |dphi| = %.3e, bound %.3e" % (tag, (k, j, i), delta, bound))
        assert delta <= bound, (tag, c, delta, bound)
    if got_phi is not None:
        reach = kw.get("smoothen", 1) + kw.get("smoothenNeg", 1)
        e = _differ(got_phi, ref_phi)
        far = [tuple(c) for c in e if not any(np.abs(c - c0).sum() <= reach for c0 in d)]
        print("%s: %d differing cell(s) after smoothing, %d of them unexplained" % (tag, len(e), len(far)), [tuple(c) for c in e])
        assert not far, (tag, far)
    return len(d)


def check_fixture_case(m, name, sc=None):
    """one fixture case on the HIP backend against the golden file, under the rule; returns HIP's phi"""
    c, I, kw = M.CASES[name], M.case_inputs(name), M.case_kwargs(name)
    sc = sc or Scene(m, c["dims"], I)
    got = sc.run(c["improved"], **kw)
    ref = GOLDEN[name + "/phi"]
    if not c["improved"]:
        util.assert_bitexact(got, ref, name)
        print("%s: 0 differing cells" % name)
        return got
    _, _, _, st = M.model_case(name)
    if c["smoothen"] or c["smoothenNeg"]:
        kw0 = dict(kw, smoothen=0, smoothenNeg=0)
        check_improved(name, sc.run(True, **kw0), GOLDEN[name + "/stage"], got, ref, st[1], st[2], kw)
    else:
        check_improved(name, got, ref, None, None, st[1], st[2], kw)
    return got


@pytest.mark.parametrize("name", list(M.CASES))
def test_hip_equals_the_reference_fixture(hip_backend, name):
    import manta as m
    check_fixture_case(m, name)


# the largest is what the model still finishes in a few seconds: crowded cells of 40 to 65 particles, long empty stretches, sizes
# that are no multiple of the block, r = 1 and r = 2, both plugins, 2-D and 3-D
RANDOM = [("imp", (33, 31, 29), 201, 30000, dict(radiusFactor=1.0, smoothen=1, smoothenNeg=1)),
          ("avg", (37, 19, 23), 202, 12000, dict(radiusFactor=1.5, smoothen=2, smoothenNeg=1)),
          ("imp", (130, 67, 1), 203, 9000, dict(radiusFactor=1.0, smoothen=0, smoothenNeg=2, t_low=0.9, t_high=1.2)),
          ("avg", (61, 50, 1), 204, 4000, dict(radiusFactor=2.0, smoothen=0, smoothenNeg=0))]


@pytest.mark.parametrize("kind,dims,seed,n,kw", RANDOM, ids=["%s-%dx%dx%d" % (r[0], *r[1]) for r in RANDOM])
def test_hip_equals_the_model_on_random_inputs(hip_backend, kind, dims, seed, n, kw):
    import manta as m
    I = M.random_inputs(dims, seed, n)
    improved = kind == "imp"
    st = M.gather(dims, I["pos"], I["pflag"], kw["radiusFactor"], I["ptype"], I["exclude"])
    assert st[3]["max_per_cell"] >= 40 and st[3]["hit"] < 0.7 * st[0].size
    want, _ = M.particle_levelset(dims, I["pos"], I["pflag"], improved, ptype=I["ptype"], exclude=I["exclude"], stage=st, **kw)
    sc = Scene(m, dims, I)
    got = sc.run(improved, **kw)
    if not improved:
        util.assert_bitexact(got, want, kind)
        return
    kw0 = dict(kw, smoothen=0, smoothenNeg=0)
    want0, _ = M.particle_levelset(dims, I["pos"], I["pflag"], True, ptype=I["ptype"], exclude=I["exclude"], stage=st, **kw0)
    check_improved("random %s" % (dims,), sc.run(True, **kw0), want0, got, want, st[1], st[2], kw)


@pytest.mark.parametrize("dims", [(12, 10, 9), (14, 11, 1)])
def test_no_particles(hip_backend, dims):
    import manta as m
    I = dict(pos=np.zeros((0, 3), np.float32), pflag=np.zeros(0, np.int32))
    sc = Scene(m, dims, I)
    assert sc.pp.pySize() == 0 and sc.pindex.size() == 0
    for improved in (False, True):
        for sm in ((0, 0), (1, 1)):
            want, _ = M.particle_levelset(dims, I["pos"], I["pflag"], improved, smoothen=sm[0], smoothenNeg=sm[1])
            util.assert_bitexact(sc.run(improved, smoothen=sm[0], smoothenNeg=sm[1]), want, "empty %s %s" % (improved, sm))
    radius = M.radius_of(dims, 1.0)[0]
    got = sc.run(False, smoothen=0, smoothenNeg=0)
    inner = got[1:-1, 1:-1, 1:-1] if dims[2] > 1 else got[:, 1:-1, 1:-1]
    assert (inner == radius).all() and got[0, 0, 0] == np.float32(0.5) and got[-1, -1, -1] == np.float32(0.5)


def test_calls_in_a_row_reuse_the_scratch_grids(hip_backend):
    import manta as m
    name, other = "imp/b3_r1_j05_s11", "avg/b3_r1_j05_s11"       # the same particles
    sc = Scene(m, M.CASES[name]["dims"], M.case_inputs(name))
    s = sc.s
    first = check_fixture_case(m, name, sc)
    live = s._live
    pooled = {k: len(v) for k, v in s._pool.items()}
    check_fixture_case(m, other, sc)                             # fewer scratch grids, another buffer parity
    second = check_fixture_case(m, name, sc)
    assert s._live == live and {k: len(v) for k, v in s._pool.items()} == pooled       # taken from the pool and given back
    util.assert_bitexact(first, second, "the same call twice")
    check_fixture_case(m, "imp/b2_r1_j20_s13")                   # another solver size on the same device right after


class _Parted(Exception):
    pass


@pytest.mark.parametrize("name", list(M.LOOPS))
def test_flip_loop_equals_the_recorded_reference_run(hip_backend, name):
    """scenes/flip02_surface.py's step at 32^3 (dam break, no adjustNumber, no mesh), 10 steps, with the level set under test before
    extrapolateLsSimple and solvePressure(phi=phi)"""
    import manta as m
    improved = M.LOOPS[name]["improved"]
    crc_ref = GOLDEN[name + "/crc"]
    seen = []

    def after_levelset(t, phi, pp, pindex, gpi, flags):
        got = phi.to_numpy()
        crc = zlib.crc32(np.ascontiguousarray(got, np.float32).tobytes()) & 0xffffffff
        seen.append(crc)
        if crc == int(crc_ref[t]):
            return
        # phi left the reference at this step: everything before was bit-identical, so the particles are the reference's, and
        # the model (bit-identical to the reference, tests/test_partls_model.py) stands in for the reference run at this step
        assert improved, "averagedParticleLevelset differs from the reference at step %d" % t
        dims = (M.LOOP_RES,) * 3
        pos, pflag = pp.get_positions(), pp.flag[:pp.np].cpu().numpy()
        st = M.gather(dims, pos, pflag, 1.0)
        ref, _ = M.particle_levelset(dims, pos, pflag, True, stage=st)
        ref0, _ = M.particle_levelset(dims, pos, pflag, True, smoothen=0, smoothenNeg=0, stage=st)
        assert zlib.crc32(ref.tobytes()) & 0xffffffff == int(crc_ref[t]), "the model does not reproduce the recorded step %d" % t
        stage = phi.parent.create(m.LevelsetGrid)
        m.improvedParticleLevelset(pp, pindex, flags, gpi, stage, 1.0, 0, 0)
        print("%s: phi leaves the reference at step %d, first cell %s" % (name, t, tuple(_differ(got, ref)[0])))
        nd = check_improved("%s step %d" % (name, t), stage.to_numpy(), ref0, got, ref, st[1], st[2], dict(smoothen=1, smoothenNeg=1))
        assert nd == 1
        raise _Parted()

    try:
        out = M.flip_loop(m, improved, after_levelset=after_levelset)
    except _Parted:
        print("%s: the trajectories part under the stage rule; steps before: %d" % (name, len(seen) - 1))
        return
    print("%s: 0 differing cells in %d steps" % (name, len(seen)))
    assert np.array_equal(out["iters"], GOLDEN[name + "/iters"]), (out["iters"], GOLDEN[name + "/iters"])
    assert int(out["np"][0]) == int(GOLDEN[name + "/np"][0])
    for k in ("phi", "vel", "pos"):
        util.assert_bitexact(out[k], GOLDEN[name + "/" + k], name + "/" + k)
