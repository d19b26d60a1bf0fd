"""Narrow-band FLIP on the MI355X: adjustNumber (rounds, compress, seeding, pdata initialisation), combineGridVel, setBoundNeumann and
initFromFlags through the package on the HIP backend, against the reference fixture tests/golden/nbflip.npz (how each array was
recorded: tests/test_nbflip_model.py) and against the numpy model tests/nbflip_model.py on seeded random inputs."""
import ctypes
import os

import numpy as np
import pytest

import nbflip_model as M
import util

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nbflip.npz"))


def _solver(m, dims):
    return m.Solver(name="nb", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)


def _grid(s, cls, arr):
    g = s.create(cls)
    g.from_numpy(arr)
    return g


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    util.assert_bitexact(got, want, what)


def _run_device(m, I, calls, dims):
    """the calls of a case on the device; returns the state after every call"""
    from mantaflow_amd import plugins
    s = _solver(m, dims)
    p = I["parts"]
    pp, chans, keep = M.parts_to_device(m, s, p, I)
    flags, phi = _grid(s, m.FlagGrid, I["flags"]), _grid(s, m.LevelsetGrid, I["phi"])
    excl = _grid(s, m.RealGrid, I["exclude"])
    out = []
    for book, kw in calls:
        if book is not None:
            pp.mDeletes, pp.mDeleteChunk = book
        kw = dict(kw)
        kw["exclude"] = excl if kw.get("exclude") else None
        m.adjustNumber(parts=pp, vel=keep[0], flags=flags, phi=phi, **kw)
        st = M.device_state(pp, chans, plugins.adjustNumberStats["compresses"])
        st["stats"] = dict(plugins.adjustNumberStats)
        out.append(st)
    return out


# ---- 1. the per-call fixture cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,allow", M.ADJUST_RUNS)
def test_hip_adjust_number_equals_reference_fixture(hip_backend, name, allow):
    """particle order, flags, every pdata channel and (mDeletes, mDeleteChunk, number of compresses), bit for bit"""
    import manta as m
    I, calls = M.adjust_case(name, allow)
    got = _run_device(m, I, calls, M.ADJUST_CASES[name][0])
    for ci, st in enumerate(got):
        for k in ("pos", "flag", "ch0", "ch1", "ch2", "ch3", "book"):
            _same(st[k], GOLDEN["adjust/%s/%d/%d/%s" % (name, int(allow), ci, k)], "%s call %d %s" % (name, ci, k))


@pytest.mark.parametrize("name", list(M.COMBINE_CASES))
def test_hip_combine_grid_vel_equals_reference_fixture(hip_backend, name):
    import manta as m
    I = M.combine_inputs(name)
    s = _solver(m, M.COMBINE_CASES[name][0])
    vel, w, comb = _grid(s, m.MACGrid, I["vel"]), _grid(s, m.MACGrid, I["weight"]), _grid(s, m.MACGrid, I["comb"])
    phi = _grid(s, m.LevelsetGrid, I["phi"]) if I["phi"] is not None else None
    m.combineGridVel(vel=vel, weight=w, combineVel=comb, phi=phi, narrowBand=I["narrowBand"], thresh=I["thresh"])
    _same(vel.to_numpy(), GOLDEN["combine/%s/vel" % name], name + " vel")
    _same(comb.to_numpy(), GOLDEN["combine/%s/comb" % name], name + " combineVel")


@pytest.mark.parametrize("which", list(M.NEUMANN_DIMS))
def test_hip_grid_ops_equal_reference_fixture(hip_backend, which):
    import manta as m
    s = _solver(m, M.NEUMANN_DIMS[which])
    r, v = M.neumann_inputs(which)
    for w in (0, 1, 2):
        gr, gv, gi = _grid(s, m.RealGrid, r), _grid(s, m.VecGrid, v), _grid(s, m.IntGrid, r.view(np.int32))
        gr.setBoundNeumann(w); gv.setBoundNeumann(w); gi.setBoundNeumann(w)
        _same(gr.to_numpy(), GOLDEN["neumann/%s/%d/real" % (which, w)], "real w%d" % w)
        _same(gv.to_numpy(), GOLDEN["neumann/%s/%d/vec" % (which, w)], "vec w%d" % w)
        _same(gi.to_numpy().view(np.float32), GOLDEN["neumann/%s/%d/real" % (which, w)], "int w%d" % w)
    fl = _grid(s, m.FlagGrid, M.flags_inputs(which))
    for ig in (0, 1):
        phi = s.create(m.LevelsetGrid)
        phi.initFromFlags(fl, ignoreWalls=bool(ig))
        _same(phi.to_numpy(), GOLDEN["initflags/%s/%d" % (which, ig)], "initFromFlags %d" % ig)


# ---- 2. HIP = model on seeded random inputs -----------------------------------------------------------------------------------------
RANDOM = [
    # dims, seed, generator options, book, allow_compress, call arguments
    ((19, 13, 11), 101, {}, (0, 0), True, dict(minParticles=3, maxParticles=5, narrowBand=2.5)),       # rows not a multiple of 8
    ((19, 13, 11), 102, {}, (5, 30), False, dict(minParticles=8, maxParticles=16, exclude=True)),
    ((37, 29, 1), 103, {}, (0, 0), True, dict(minParticles=4, maxParticles=6, radiusFactor=1.5)),      # 2-D
    ((37, 29, 1), 104, {}, (0, 7), False, dict(minParticles=4, maxParticles=8, narrowBand=3.)),
    ((12, 10, 9), 105, dict(max_per_cell=70, dense_frac=0.5), (0, 0), True, dict(minParticles=2, maxParticles=40)),   # > 32 per cell
    ((12, 10, 9), 106, dict(max_per_cell=70, dense_frac=0.5), (0, 0), False, dict(minParticles=2, maxParticles=33)),
]


def _model_call(I, book, allow, kw):
    p = I["parts"].copy()
    p.deletes, p.chunk, p.allow_compress = book[0], book[1], allow
    kw = dict(kw)
    kw["exclude"] = I["exclude"] if kw.get("exclude") else None
    M.adjust_number(p, I["flags"], I["phi"], segmented=True, **kw)
    return p


def _compare_state(got, p, what):
    want = p.state()
    for k in want:
        _same(got[k], want[k], what + " " + k)


@pytest.mark.parametrize("case", range(len(RANDOM)))
def test_hip_adjust_number_equals_model_random(hip_backend, case):
    import manta as m
    dims, seed, opt, book, allow, kw = RANDOM[case]
    I = M.adjust_inputs(dims, seed, **opt)
    I["parts"].allow_compress = allow
    want = _model_call(I, book, allow, kw)
    got = _run_device(m, I, [(book, kw)], dims)[0]
    print("case %d: %d -> %d particles, stats %s" % (case, I["parts"].size(), want.size(), got["stats"]))
    _compare_state(got, want, "case %d" % case)
    if case in (4, 5):
        assert np.bincount(M.classify(I["parts"].pos, I["phi"], -1., M.surface_ls(True, 1.))[0].clip(0)).max() > 32


def test_hip_adjust_number_large_three_rounds_and_rerun(hip_backend):
    """at least 200 k particles, compress allowed from a fresh (0, 0) system: at least three rounds; a second run gives the same bits"""
    import manta as m
    dims = (50, 40, 36)
    I = M.adjust_inputs(dims, 107, max_per_cell=24, dense_frac=0.5, deleted_frac=0.08, outside=400)
    assert I["parts"].size() >= 200000, I["parts"].size()
    kw = dict(minParticles=4, maxParticles=6, narrowBand=4.)
    want = _model_call(I, (0, 0), True, kw)
    I["parts"].allow_compress = True
    got = _run_device(m, I, [((0, 0), kw)], dims)[0]
    again = _run_device(m, I, [((0, 0), kw)], dims)[0]
    print("large: %d -> %d particles, stats %s" % (I["parts"].size(), want.size(), got["stats"]))
    assert got["stats"]["rounds"] >= 3 and want.rounds == got["stats"]["rounds"]
    _compare_state(got, want, "large")
    for k in ("pos", "flag", "ch0", "ch1", "ch2", "ch3", "book"):
        _same(again[k], got[k], "re-run " + k)


# ---- 3. the narrow-band loops --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.LOOPS))
def test_hip_narrow_band_loop_equals_reference(hip_backend, name):
    """particle counts and CG iterations equal at every step; fields within 1e-5 relative (README's bar for fp32 fields)"""
    import manta as m
    got = M.nb_loop(m, **M.LOOPS[name])
    g = lambda k: GOLDEN["loop/%s/%s" % (name, k)]
    print("%s: counts %s (reference %s), iterations %s (reference %s)" % (name, got["counts"].tolist(), g("counts").tolist(),
                                                                         got["iters"].tolist(), g("iters").tolist()))
    errs = {k: util.rel_err(got[k], g(k)) for k in ("phi", "vel", "phiParts", "velParts")}
    exact = {k: np.array_equal(got[k].view(np.int32), g(k).view(np.int32)) for k in errs}
    print("%s: rel err %s, bit-exact %s" % (name, errs, exact))
    assert got["counts"].tolist() == g("counts").tolist()
    assert got["iters"].tolist() == g("iters").tolist()
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)
    k = int(g("pstride")[0])
    util.assert_bitexact(got["flag"][::k], g("flag"), name + " particle flags")
    for key in ("pos", "pvel"):
        e = util.rel_err(got[key][::k], g(key))
        print("%s: particles %s rel err %g, bit-exact %s" % (name, key, e, np.array_equal(got[key][::k].view(np.int32), g(key).view(np.int32))))
        assert e <= 1e-5, (key, e)


def _chain_hooks(ctx):
    """before every adjustNumber copy the device state to the model; after it the device must equal the model bit for bit"""
    box = {}

    def before(t, pp, pVel, flags, phi, vel):
        v = vel.to_numpy()
        p = M.model_from_device(pp, [pVel], [(v, True)])
        box["want"], box["args"] = p, (flags.to_numpy(), phi.to_numpy())
        box["excl"] = ctx.get("exclude")

    def after(t, pp, pVel):
        p = box["want"]
        fl, ph = box["args"]
        M.adjust_number(p, fl, ph, segmented=True, **dict(ctx["kw"], exclude=box["excl"]))
        from mantaflow_amd import plugins
        _compare_state(M.device_state(pp, [pVel], plugins.adjustNumberStats["compresses"]), p, "adjustNumber of step %d" % t)
        ctx["checked"] = ctx.get("checked", 0) + 1
    return before, after


def test_hip_narrow_band_loop_every_adjust_number_equals_model(hip_backend):
    """the chain test: drift upstream of adjustNumber cannot hide a wrong call"""
    import manta as m
    cfg = M.LOOPS["loop3d"]
    ctx = dict(kw=dict(minParticles=8, maxParticles=16, narrowBand=float(M.NARROW_BAND)))
    before, after = _chain_hooks(ctx)
    M.nb_loop(m, before_adjust=before, after_adjust=after, **cfg)
    assert ctx["checked"] == cfg["steps"]


def test_hip_obstacle_narrow_band_step(hip_backend):
    """the step of the reference's obstacle FLIP scene: narrow band + updateFractions / setObstacleFlags / fraction-mode setWallBcs /
    solvePressure(phi, fractions) / adjustNumber(exclude=phiObs), 5 steps at res 32: fields stay finite, particles remain, and every
    adjustNumber call equals the model chain.  No bound on how deep a particle may sit is asserted."""
    import manta as m
    res, band, minP = 32, 4, 8
    gs = m.vec3(res, res, res)
    s = m.Solver(name="obs", gridSize=gs, dim=3)
    s.timestep = 0.8
    flags, phi, phiParts, phiObs = s.create(m.FlagGrid), s.create(m.LevelsetGrid), s.create(m.LevelsetGrid), s.create(m.LevelsetGrid)
    vel, velOld, velParts, fractions = (s.create(m.MACGrid) for _ in range(4))
    pressure, tmpVec3 = s.create(m.RealGrid), s.create(m.VecGrid)
    pp = s.create(m.BasicParticleSystem)
    pVel = pp.create(m.PdataVec3)
    pindex, gpi = s.create(m.ParticleIndexSystem), s.create(m.IntGrid)
    flags.initDomain(boundaryWidth=1, phiWalls=phiObs)
    phi.setConst(999.)
    phi.join(m.Box(parent=s, p0=gs * m.vec3(0, 0, 0), p1=gs * m.vec3(1.0, 0.3, 1)).computeLevelset())
    phi.join(m.Box(parent=s, p0=gs * m.vec3(0.1, 0, 0), p1=gs * m.vec3(0.2, 0.75, 1)).computeLevelset())
    phiObs.join(m.Sphere(parent=s, center=gs * m.vec3(0.66, 0.3, 0.5), radius=res * 0.2).computeLevelset())
    flags.updateFromLevelset(phi)
    phi.subtract(phiObs)
    m.sampleLevelsetWithParticles(phi=phi, flags=flags, parts=pp, discretization=2, randomness=0.05)
    m.updateFractions(flags=flags, phiObs=phiObs, fractions=fractions, boundaryWidth=1)
    m.setObstacleFlags(flags=flags, phiObs=phiObs, fractions=fractions)
    ctx = dict(kw=dict(minParticles=minP, maxParticles=2 * minP, narrowBand=float(band)), exclude=phiObs.to_numpy())
    before, after = _chain_hooks(ctx)
    for t in range(5):
        pp.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4, deleteInObstacle=False, stopInObstacle=False)
        m.pushOutofObs(parts=pp, flags=flags, phiObs=phiObs)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=phi, order=1)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2)
        m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
        m.unionParticleLevelset(pp, pindex, flags, gpi, phiParts)
        phi.addConst(1.)
        phi.join(phiParts)
        m.extrapolateLsSimple(phi=phi, distance=band + 2, inside=True)
        m.extrapolateLsSimple(phi=phi, distance=3)
        phi.setBoundNeumann(0)
        flags.updateFromLevelset(phi)
        m.mapPartsToMAC(vel=velParts, flags=flags, velOld=velOld, parts=pp, partVel=pVel, weight=tmpVec3)
        m.extrapolateMACFromWeight(vel=velParts, distance=2, weight=tmpVec3)
        m.combineGridVel(vel=velParts, weight=tmpVec3, combineVel=vel, phi=phi, narrowBand=band - 1, thresh=0)
        velOld.copyFrom(vel)
        m.addGravity(flags=flags, vel=vel, gravity=(0, -0.001, 0))
        m.extrapolateMACSimple(flags=flags, vel=vel, distance=2, intoObs=True)
        m.setWallBcs(flags=flags, vel=vel, fractions=fractions, phiObs=phiObs)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure, phi=phi, fractions=fractions)
        m.extrapolateMACSimple(flags=flags, vel=vel, distance=4, intoObs=True)
        m.setWallBcs(flags=flags, vel=vel, fractions=fractions, phiObs=phiObs)
        m.flipVelocityUpdate(vel=vel, velOld=velOld, flags=flags, parts=pp, partVel=pVel, flipRatio=0.95)
        pVel.setSource(vel, isMAC=True)
        before(t, pp, pVel, flags, phi, vel)
        m.adjustNumber(parts=pp, vel=vel, flags=flags, minParticles=minP, maxParticles=2 * minP, phi=phi, exclude=phiObs, narrowBand=band)
        after(t, pp, pVel)
        s.step()
    assert ctx["checked"] == 5
    assert pp.pySize() > 1000
    for g in (vel, phi, pressure):
        assert np.isfinite(g.to_numpy()).all()
    assert np.isfinite(pp.get_positions()).all() and np.isfinite(pVel.to_numpy()).all()


def test_hip_library_exports_every_resample_symbol():
    from mantaflow_amd import _lib
    L = ctypes.CDLL(util.HIP_LIB)
    for name in _lib.parse_header(_lib.RESAMPLE_HEADER):
        assert hasattr(L, name), name
    assert L.mf_resample_abi_version() == 1
