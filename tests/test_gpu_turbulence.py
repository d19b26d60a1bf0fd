"""GPU: the turbulence model through the package on the HIP backend: HIP = numpy model = reference fixture, bit for bit
(tests/golden/turbulence.npz; how each array was produced: tools/record_turbulence.py; arrays of more than
turbulence_model.FULL_LIMIT elements are in the fixture as SHA-256 digests, so the device result is also compared, word by word, with
the model's array).  Outputs are pre-filled with the values the fixture's caller grids held (border cells must keep them) and, in a
second call, with NaN; the solver's pool scratch is pre-filled with NaN.

The particle cases start from the recorded process-wide state (stream position, clock, inflow offset), so each is a test of its own;
the model's side of them is computed once per session.  The loop is tools/tests/test_2025_turb.py's at 40 x 20 x 20 against a recorded
reference run."""
import os

import numpy as np
import pytest

import turbulence_model as M

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "turbulence.npz"))
f32 = np.float32


def _solver(m, dims, dt=M.DT):
    s = m.Solver(name="t", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)
    s.timestep = dt
    return s


def _grid(s, cls, arr):
    g = s.create(cls)
    g.from_numpy(arr)
    return g


def _poison_pool(s):
    """the next scratch grids the plugins take from the solver's pool hold NaN"""
    import torch
    for kind, ncomp in (("real", 1), ("vec", 3)):
        for _ in range(2):
            s._pool.setdefault(kind, []).append(torch.full((ncomp * s.ncells,), float("nan"), dtype=torch.float32, device=s.device))


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


# ---------------------------------------------------------------------------------------------------------------------------------
# the four plugins
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_strain", (True, False))
@pytest.mark.parametrize("name", M.PRODUCTION_CASES)
def test_production(hip_backend, name, with_strain):
    import manta as m
    I = M.ke_inputs(name, nan=True)
    sh = M.shape_of(I["dims"])
    model = M.run_production(name, with_strain)
    interior = M.interior_mask(sh)
    for fill in ("fixture", "nan"):
        s = _solver(m, I["dims"])
        vel, k, eps = _grid(s, m.MACGrid, I["vel"]), _grid(s, m.RealGrid, I["k"]), _grid(s, m.RealGrid, I["eps"])
        pre = {key: (M.prefill(name, key) if fill == "fixture" else np.full(sh, np.nan, f32)) for key in ("prod", "nuT", "strain")}
        out = {key: _grid(s, m.RealGrid, a) for key, a in pre.items()}
        _poison_pool(s)
        live = s._live
        m.KEpsilonComputeProduction(vel=vel, k=k, eps=eps, prod=out["prod"], nuT=out["nuT"], strain=out["strain"] if with_strain else None,
                                    pscale=M.PSCALE)
        assert s._live == live                               # one kernel, no scratch
        got = dict(k=k.to_numpy(), eps=eps.to_numpy(), prod=out["prod"].to_numpy(), nuT=out["nuT"].to_numpy(), strain=out["strain"].to_numpy())
        if fill == "fixture":
            for key in model:
                check("production/%s/%s" % (name, key), got[key], model[key])
        else:
            for key in ("k", "eps"):
                bits_equal(key, got[key], model[key])
            for key in ("prod", "nuT") + (("strain",) if with_strain else ()):
                bits_equal(key + " interior", got[key][interior], model[key][interior])
                assert np.isnan(got[key][~interior]).all(), key          # border cells keep the caller's values
        if not with_strain:
            bits_equal("strain untouched", got["strain"], pre["strain"])


@pytest.mark.parametrize("name", M.SOURCES_CASES)
def test_sources_and_bcs(hip_backend, name):
    import manta as m
    I = M.ke_inputs(name)
    s = _solver(m, I["dims"])
    k, eps, prod = (_grid(s, m.RealGrid, I[key]) for key in ("k", "eps", "prod"))
    m.KEpsilonSources(k=k, eps=eps, prod=prod)
    model = M.run_sources(name)
    check("sources/%s/k" % name, k.to_numpy(), model["k"])
    check("sources/%s/eps" % name, eps.to_numpy(), model["eps"])
    bits_equal("prod", prod.to_numpy(), I["prod"])
    flags = _grid(s, m.FlagGrid, I["flags"])
    for fill in (False, True):
        k.from_numpy(I["k"]), eps.from_numpy(I["eps"])
        m.KEpsilonBcs(flags=flags, k=k, eps=eps, intensity=M.BCS["intensity"], nu=M.BCS["nu"], fillArea=fill)
        model = M.run_bcs(name, fill)
        check("bcs/%s/%d/k" % (name, fill), k.to_numpy(), model["k"])
        check("bcs/%s/%d/eps" % (name, fill), eps.to_numpy(), model["eps"])


@pytest.mark.parametrize("with_vel", (False, True))
@pytest.mark.parametrize("name", M.GRADDIFF_CASES)
def test_gradient_diffusion_twice(hip_backend, name, with_vel):
    """two calls in a row: the swap of the field with its scratch grid leaves nothing stale"""
    import manta as m
    I = M.graddiff_inputs(name)
    s = _solver(m, I["dims"])
    k, eps, nuT, vel = _grid(s, m.RealGrid, I["k"]), _grid(s, m.RealGrid, I["eps"]), _grid(s, m.RealGrid, I["nuT"]), _grid(s, m.MACGrid, I["vel"])
    live = s._live
    for _ in range(2):
        _poison_pool(s)
        m.KEpsilonGradientDiffusion(k=k, eps=eps, nuT=nuT, sigmaU=M.SIGMA_U, vel=vel if with_vel else None)
        assert s._live == live                               # the scratch went back to the pool
    model = M.run_graddiff(name, with_vel)
    check("graddiff/%s/%d/k" % (name, with_vel), k.to_numpy(), model["k"])
    check("graddiff/%s/%d/eps" % (name, with_vel), eps.to_numpy(), model["eps"])
    if with_vel:
        check("graddiff/%s/1/vel" % name, vel.to_numpy(), model["vel"])
    else:
        bits_equal("vel untouched", vel.to_numpy(), I["vel"])
    bits_equal("nuT untouched", nuT.to_numpy(), I["nuT"])


@pytest.mark.parametrize("name", M.DIAG_CASES)
def test_diagnostics(hip_backend, name):
    import manta as m
    dims = M.DIMS[name]
    sh = M.shape_of(dims)
    s = _solver(m, dims)
    vel = _grid(s, m.MACGrid, M.rand_vel(name, 2.0))
    mag, vort = _grid(s, m.RealGrid, M.prefill(name, "mag")), _grid(s, m.VecGrid, M.diag_prefill_vec(name))
    nrm = _grid(s, m.RealGrid, np.full(sh, np.nan, f32))
    _poison_pool(s)
    live = s._live
    m.computeStrainRateMag(vel, mag)
    m.computeVorticity(vel, vort, nrm)
    assert s._live == live                                   # fused: no centred-velocity grid, no curl grid
    model = M.run_diagnostics(name)
    check("diag/%s/mag" % name, mag.to_numpy(), model["mag"])
    check("diag/%s/vort" % name, vort.to_numpy(), model["vort"])
    check("diag/%s/norm" % name, nrm.to_numpy(), model["norm"])
    for comp in range(3):
        c = _grid(s, m.RealGrid, np.full(sh, np.nan, f32))
        m.getCurl(vel, c, comp)
        check("diag/%s/curl%d" % (name, comp), c.to_numpy(), model["curl%d" % comp])
    vort2 = _grid(s, m.VecGrid, M.diag_prefill_vec(name))
    m.computeVorticity(vel, vort2)                           # norm = None
    bits_equal("vorticity without norm", vort2.to_numpy(), model["vort"])


# ---------------------------------------------------------------------------------------------------------------------------------
# turbulence particles
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def particle_model():
    """the model's side of every particle case, in the recorded order on one continuing state (CPU; advectInGrid from the checker)"""
    from mantaflow_amd import _lib
    _lib.reset()
    tile, params = M.noise_tile_and_params(M.PDIMS)          # the CPU checker's tile: bit-exact with the device's (tests/test_gpu_parity.py)
    _lib.reset()
    st, runs = M.State(), {}
    for name in M.PARTICLE_ORDER:
        runs[name] = M.run_particle_case(name, st, tile, params)
    return runs


@pytest.mark.parametrize("name", M.PARTICLE_ORDER)
def test_particle_case(particle_model, hip_backend, name):
    import manta as m
    state, sizes, cursors = M.run_particle_case_pkg(m, name, GOLDEN["parts/%s/start" % name])
    mstate, msizes, mcursors = particle_model[name]
    assert list(sizes) == list(msizes) == list(GOLDEN["parts/%s/sizes" % name])           # size after every call
    assert list(cursors) == list(mcursors) == list(GOLDEN["parts/%s/cursors" % name])     # stream position after every call
    for c in M.CHANNELS:                                                                   # order and every channel
        check("parts/%s/%s" % (name, c), state[c], mstate[c])
    m.resetTurbulenceParticleState()


def test_delete_leaves_a_slot_outside_the_grid_alone(hip_backend):
    """outside the contract (the reference reads outside the flag grid): the kernel treats such a slot as "not an obstacle\""""
    import manta as m
    m.resetTurbulenceParticleState()
    s = _solver(m, M.PDIMS, M.PDT)
    flags = _grid(s, m.FlagGrid, M.particle_grids()[0])
    turb = s.create(m.TurbulenceParticleSystem, noise=s.create(m.NoiseField))
    turb.seed(M.pkg_shape(m, s, "box", M.FREE_BOX), 6)
    before = turb.channels_to_numpy()
    for slot, p in ((1, (-7.0, 4.0, 4.0)), (3, (4.0, 4.0, 1e9)), (4, (float("nan"), 4.0, 4.0))):
        for c in range(3):
            turb.pos[c * turb.cap + slot] = p[c]
            before["pos"][slot, c] = p[c]
    turb.deleteInObstacle(flags)
    after = turb.channels_to_numpy()
    assert turb.pySize() == 6
    for c in M.CHANNELS:
        bits_equal(c, after[c], before[c])
    m.resetTurbulenceParticleState()


# ---------------------------------------------------------------------------------------------------------------------------------
# the loop of tools/tests/test_2025_turb.py
# ---------------------------------------------------------------------------------------------------------------------------------
def test_loop_against_the_recorded_reference_run(hip_backend):
    import manta as m
    from mantaflow_amd import core
    C = M.LOOP
    start = GOLDEN["loop/start"]
    st = M.State.from_snapshot(start)
    core._set_turbulence_particle_state(int(start[0]), st.ctime, st.inflow)
    g = M.setup_loop_pkg(m, C["res"], C["dt"])
    assert int(((g["flags"].to_numpy()[1:-1, 1:-1, 1:-1] & 2) != 0).sum()) == GOLDEN["loop/obstacle_cells"][0]      # the 16 spheres
    per_step = np.array([M.step_loop_pkg(m, g) for _ in range(C["steps"])], np.int64)
    print("per step (particles, CG iterations):", per_step.tolist())
    assert per_step.tolist() == GOLDEN["loop/per_step"].tolist()
    for key in ("k", "eps", "prod", "nuT", "strain", "vel", "pressure"):
        msg = M.same_as_fixture(GOLDEN, "loop/" + key, g[key].to_numpy())
        assert msg is None, msg
    parts = g["turb"].channels_to_numpy()
    for c in M.CHANNELS:
        msg = M.same_as_fixture(GOLDEN, "loop/parts/" + c, parts[c])
        assert msg is None, msg
    m.resetTurbulenceParticleState()
