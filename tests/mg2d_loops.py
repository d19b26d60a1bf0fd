"""The three recorded loops of tests/golden/mg2d.npz, written against the `manta` module: tests/test_gpu_mg2d.py runs them on the HIP
library, tools/mg2d_record.cpp states the same calls (same arguments, same order) against the reference's classes.  Each function
expects the 2-D multigrid switch to be on (mantaflow_amd.multigrid2d.setMultigrid2D) and returns what the fixture holds.  plume and
flip take another preconditioner in place of the scene's: with PcMIC (plain CG on a 2-D solver) they run on the CPU checker backend,
which is how tools/record_mg2d.py holds this text against the recorder's own statement of the same loops."""
import numpy as np

from mg2d_cases import FLIP, GUIDING, PLUME


def plume(preconditioner=None):
    """(a) scenes/plume_2d.py's loop at 64 x 64 for 4 steps, its solvePressure with preconditioner = PcMGDynamic"""
    import manta as m
    from manta import vec3
    pc = m.PcMGDynamic if preconditioner is None else preconditioner
    res = PLUME["res"]
    gs = vec3(res, res, 1)
    s = m.Solver(name="main", gridSize=gs, dim=2)
    s.timestep = 1.0
    flags, vel, density, pressure = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.RealGrid), s.create(m.RealGrid)
    flags.initDomain(boundaryWidth=1)
    flags.fillGrid()
    m.setOpenBound(flags, 1, "yY", m.FlagOutflow | m.FlagEmpty)
    source = s.create(m.Cylinder, center=gs * vec3(0.5, 0.1, 0.5), radius=res * 0.14, z=gs * vec3(0, 0.02, 0))
    cg = []
    for t in range(PLUME["steps"]):
        source.applyToGrid(grid=density, value=1)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=density, order=2)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2)
        m.resetOutflow(flags=flags, real=density)
        m.setWallBcs(flags=flags, vel=vel)
        m.addBuoyancy(density=density, vel=vel, gravity=vec3(0, -4e-3, 0), flags=flags)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure, preconditioner=pc)
        cg.append(m.lastCgStats()["iterations"])
        assert s._mg is None, "a hierarchy was left behind"      # PcMGDynamic releases its own
        s.step()
    return dict(cg=cg, vel=vel.to_numpy(), density=density.to_numpy(), pressure=pressure.to_numpy())


def guiding():
    """(b) scenes/guiding_2d.py's loop at res0 = 40, scale = 1 for 2 steps as the scene ships it: PcMGStatic, zeroPressureFixing"""
    import manta as m
    from manta import vec3
    res0, scale = GUIDING["res0"], GUIDING["scale"]
    res = res0 * scale
    gs = vec3(res, res, 1)
    s = m.Solver(name="main", gridSize=gs, dim=2)
    s.timestep = 2.0 / scale
    beta, tau = 2, 1.0
    sigma, theta = 0.99 / tau, 1.0
    flags, vel, velT = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.MACGrid)
    density, pressure, W = s.create(m.RealGrid), s.create(m.RealGrid), s.create(m.RealGrid)
    flags.initDomain(boundaryWidth=1)
    flags.fillGrid()
    source = s.create(m.Cylinder, center=gs * vec3(0.5, 0.2, 0.5), radius=gs.y * 0.14, z=gs * vec3(0, 0.02 * 1.5, 0))
    m.getSpiralVelocity(flags=flags, vel=velT, strength=0.5 * scale)
    m.setGradientYWeight(W=W, minY=0, maxY=res / 2, valAtMin=1, valAtMax=1)
    m.setGradientYWeight(W=W, minY=res / 2, maxY=res, valAtMin=5, valAtMax=5)
    m.releaseBlurPrecomp()
    pd, cg = [], []
    try:
        for t in range(GUIDING["steps"]):
            m.resetOutflow(flags=flags, real=density)
            source.applyToGrid(grid=density, value=1)
            m.advectSemiLagrange(flags=flags, vel=vel, grid=density, order=2)
            m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2)
            m.setWallBcs(flags=flags, vel=vel)
            m.addBuoyancy(density=density, vel=vel, gravity=vec3(0, 0.25 * scale * -4e-3, 0), flags=flags)
            m.PD_fluid_guiding(vel=vel, velT=velT, flags=flags, weight=W, blurRadius=beta, pressure=pressure,
                               tau=tau, sigma=sigma, theta=theta, preconditioner=m.PcMGStatic, zeroPressureFixing=True)
            st = m.lastGuidingStats()
            pd.append(st["iterations"])
            cg += st["cg_iterations"]
            m.setWallBcs(flags=flags, vel=vel)
            s.step()
        setups = s._mg.info()["setups"] if s._mg is not None else None
    finally:
        m.releaseBlurPrecomp()
        m.releaseMG(s)
    return dict(pd=pd, cg=cg, setups=setups, vel=vel.to_numpy(), density=density.to_numpy(), pressure=pressure.to_numpy())


def flip_particles():
    """the dam's particles: a 2 x 2 lattice per cell of the box (0 .. 0.4 res) x (0 .. 0.6 res) behind the wall cells, jittered by a
    seeded generator; [3][np] float32, z = 0.5"""
    res = FLIP["res"]
    rng = np.random.default_rng(48)
    ii, jj = np.meshgrid(np.arange(1, int(0.4 * res)), np.arange(1, int(0.6 * res)), indexing="xy")
    cells = np.stack([ii.ravel(), jj.ravel()], 0).astype(np.float64)
    sub = np.array([[0.25, 0.75, 0.25, 0.75], [0.25, 0.25, 0.75, 0.75]])
    xy = (cells[:, :, None] + sub[:, None, :]).reshape(2, -1)
    xy = xy + rng.uniform(-0.1, 0.1, xy.shape)
    pos = np.concatenate([xy, np.full((1, xy.shape[1]), 0.5)], 0).astype(np.float32)
    return np.ascontiguousarray(pos)


def flip(preconditioner=None):
    """(c) a 2-D FLIP dam break at 48 x 48 for 4 steps (flip01_simple.py's dam, flip02_surface.py's loop without resampling and
    mesh) with solvePressure(phi=phi, preconditioner=PcMGStatic) and a releaseMG in the middle"""
    import manta as m
    import torch
    from manta import vec3
    pc = m.PcMGStatic if preconditioner is None else preconditioner
    res = FLIP["res"]
    gs = vec3(res, res, 1)
    s = m.Solver(name="main", gridSize=gs, dim=2)
    s.timestep = 0.5
    flags, phi = s.create(m.FlagGrid), s.create(m.LevelsetGrid)
    vel, velOld, pressure, tmpVec3 = s.create(m.MACGrid), s.create(m.MACGrid), s.create(m.RealGrid), s.create(m.VecGrid)
    pp = s.create(m.BasicParticleSystem)
    pVel = pp.create(m.PdataVec3)
    pindex, gpi = s.create(m.ParticleIndexSystem), s.create(m.IntGrid)
    flags.initDomain(boundaryWidth=0)
    fluidbox = m.Box(parent=s, p0=gs * vec3(0, 0, 0), p1=gs * vec3(0.4, 0.6, 1))
    flags.updateFromLevelset(fluidbox.computeLevelset())
    pos = flip_particles()
    pp.resizeAll(pos.shape[1])
    for c in range(3):
        pp.pos[c * pp.cap:c * pp.cap + pp.np] = torch.from_numpy(pos[c]).to(pp.pos.device)
    pp.flag[:pp.np] = 0
    pVel.setConst(vec3(0, 0, 0))
    cg, setups = [], []
    try:
        for t in range(FLIP["steps"]):
            pp.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4, deleteInObstacle=False)
            m.mapPartsToMAC(vel=vel, flags=flags, velOld=velOld, parts=pp, partVel=pVel, weight=tmpVec3)
            m.extrapolateMACFromWeight(vel=vel, distance=2, weight=tmpVec3)
            m.markFluidCells(parts=pp, flags=flags)
            m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
            m.unionParticleLevelset(pp, pindex, flags, gpi, phi, 1.0)
            m.extrapolateLsSimple(phi=phi, distance=4, inside=True)
            m.addGravity(flags=flags, vel=vel, gravity=vec3(0, -0.002, 0))
            m.setWallBcs(flags=flags, vel=vel)
            m.solvePressure(flags=flags, vel=vel, pressure=pressure, phi=phi, preconditioner=pc)
            cg.append(m.lastCgStats()["iterations"])
            setups.append(s._mg.info()["setups"] if s._mg is not None else None)
            m.setWallBcs(flags=flags, vel=vel)
            m.extrapolateMACSimple(flags=flags, vel=vel, distance=1)
            m.flipVelocityUpdate(vel=vel, velOld=velOld, flags=flags, parts=pp, partVel=pVel, flipRatio=0.97)
            if t + 1 == FLIP["release_after"]:
                m.releaseMG(s)
                assert s._mg is None
            s.step()
    finally:
        m.releaseMG(s)
    assert pp.np == pos.shape[1]
    a = pp.pos.detach().cpu().numpy()
    out_pos = np.stack([a[c * pp.cap:c * pp.cap + pp.np] for c in range(3)], 0)
    v = pVel.data.detach().cpu().numpy()
    out_vel = np.stack([v[c * pVel.cap:c * pVel.cap + pp.np] for c in range(3)], 0)
    return dict(cg=cg, setups=setups, vel=vel.to_numpy(), phi=phi.to_numpy(), pressure=pressure.to_numpy(), flags=flags.to_numpy(),
                pos=out_pos[:, ::7].copy(), pvel=out_vel[:, ::7].copy())
