"""GPU: the vortex particle family on the MI355X (include/open/manta_hip_vortex.h) against the numpy model, against itself stage by
stage, and against the reference's recorded outputs (tests/golden/vortex.npz).

1. mf_vortex_velocity against the model, per target and component within 2^-23 * (sum |t_i| + n * max |S_j|): one fp32 ulp per term whose
   fp64 `exp` rounded the other way, plus one ulp of the running sum per later addition.  The number of targets that are not
   bit-identical and the largest error as a fraction of the bound are printed; zero is expected.
2. every integration mode of advectSelf and applyToMesh: the fused call is bit-identical to the same stages composed from
   mf_vortex_velocity plus the model's update arithmetic applied to the device's own u.
3. the end state of every mode against the recorded reference, asserted where item 1 found no differing target.
4. densityFromLevelset, the recorded loop (VPseedK41, advectSelf, advectInGrid with deletions, compress), calls in a row, empty sets.
Outputs and pool scratch are pre-filled with NaN."""
import ctypes
import os

import numpy as np
import pytest

import vortex_model as M

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vortex.npz"))
f32 = np.float32
DT = 0.5
DIMS = (12, 10, 8)

ALL = list(M.CASES) + list(M.EXTRA_CASES)      # the fixture's cases and seeded ones beside them
FIXTURE = list(M.CASES)
_checked = {}


def _solver(m, dims=DIMS, dt=DT):
    s = m.Solver(name="v", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)
    s.timestep = dt
    return s


def _poison_pool(s):
    """the scratch the next calls take from the solver's pool holds NaN"""
    held = [s._alloc("vec", zero=False) for _ in range(4)]
    for t in held:
        t.fill_(float("nan"))
        s._release("vec", t)


def _system(m, s, P):
    import torch
    vp = s.create(m.VortexParticleSystem)
    vp.set_numpy(P["pos"], P["vorticity"], P["sigma"], P["flag"])
    vp._pos2 = torch.full((3 * vp.cap,), float("nan"), dtype=torch.float32, device=s.device) if vp.cap else None
    return vp


def _device_velocity(s, vp, tpos, tflag, tmask):
    """mf_vortex_velocity for host targets tpos[nT][3], tflag[nT] (None: the system's own particles) -> u[nT][3]"""
    import torch
    from mantaflow_amd.core import _ptr
    dev = s.device
    if tpos is None:
        nT, tcap, tp, tf = vp.np, vp.cap, vp.pos, vp.flag
    else:
        nT = tcap = tpos.shape[0]
        tp = torch.from_numpy(np.ascontiguousarray(tpos.T)).to(dev).reshape(-1)
        tf = torch.from_numpy(np.ascontiguousarray(tflag, np.int32)).to(dev)
    need = ctypes.c_int64(0)
    s.lib.call("mf_vortex_scratch_bytes", vp.np, ctypes.byref(need))
    tmp = torch.full(((need.value + 3) // 4 + 4,), float("nan"), dtype=torch.float32, device=dev)
    u = torch.full((3 * max(nT, 1),), float("nan"), dtype=torch.float32, device=dev)
    s.lib.call("mf_vortex_velocity", nT, tcap, _ptr(tp), _ptr(tf), tmask, vp.np, vp.cap, _ptr(vp.pos), _ptr(vp.flag), vp.vorticity.ptr,
               vp.sigma.ptr, float(f32(vp._scale_dt)), _ptr(tmp), tmp.numel() * 4, max(nT, 1), _ptr(u), s.stream)
    s.sync()
    return np.ascontiguousarray(u.cpu().numpy().reshape(3, max(nT, 1))[:, :nT].T)


def _velocity_check(name):
    """item 1 for one case -> (targets not bit-identical, largest |error| / bound); cached"""
    if name in _checked:
        return _checked[name]
    import manta as m
    I = M.case_inputs(name)
    s = _solver(m)
    vp = _system(m, s, I["P"])
    vp._scale_dt = I["scale"]
    tp, tz = M.case_targets(I)
    if I["kind"] == "self":
        got = _device_velocity(s, vp, None, None, M.PDELETE)
    else:
        got = _device_velocity(s, vp, tp, I["nflags"], M.NF_FIXED)
    want, bound = M.case_velocity(name, bound=True)
    assert got.shape == want.shape and not np.isnan(got).any()
    differ = int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()) if got.size else 0
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    with np.errstate(all="ignore"):
        frac = float(np.nanmax(np.where(err > 0, err / bound, 0.0))) if err.size else 0.0
    print("velocity %s: %d of %d targets not bit-identical, largest error %.3g of the bound" % (name, differ, got.shape[0], frac))
    assert (err <= bound).all(), "%s: %d components beyond the bound" % (name, int((err > bound).sum()))
    _checked[name] = (differ, frac)
    return _checked[name]


@pytest.mark.parametrize("name", ALL)
def test_velocity_against_the_model(hip_backend, name):
    _velocity_check(name)


def _run_fused(m, I, mode):
    s = _solver(m)
    _poison_pool(s)
    vp = _system(m, s, I["P"])
    scale = float(f32(I["scale"] / f32(DT)))
    assert f32(f32(scale) * f32(DT)) == I["scale"]
    live = s._live
    if I["kind"] == "self":
        vp.advectSelf(scale=scale, integrationMode=mode)
        got = vp.numpy()["pos"]
    else:
        mesh = s.create(m.Mesh)
        mesh.set_numpy(I["nodes"], flags=I["nflags"])
        vp.applyToMesh(mesh, scale=scale, integrationMode=mode)
        got = mesh.nodes_numpy()[0]
        after = vp.numpy()
        for ch in M.CHANNELS:                                   # the particles stay
            assert np.array_equal(after[ch].view(np.uint32), np.ascontiguousarray(I["P"][ch]).view(np.uint32)), ch
    assert s._live == live                                      # every scratch grid went back to the pool
    return got


def _run_composed(m, I, mode):
    """the same stages from mf_vortex_velocity and the model's update arithmetic on the device's own u"""
    s = _solver(m)
    P = {k: v.copy() for k, v in I["P"].items()}
    x = (P["pos"] if I["kind"] == "self" else I["nodes"]).copy()
    x0 = ut = None
    for step in M.STEPS[mode]:
        if I["kind"] == "self":
            P["pos"] = x
            vp = _system(m, s, P)
            vp._scale_dt = I["scale"]
            u = _device_velocity(s, vp, None, None, M.PDELETE)
        else:
            vp = _system(m, s, P)
            vp._scale_dt = I["scale"]
            u = _device_velocity(s, vp, x, I["nflags"], M.NF_FIXED)
        with np.errstate(all="ignore"):
            x, x0, ut = M.stage_update(step, x, u, x0, ut)
    return x


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("name", ALL)
def test_fused_call_is_its_stages_and_ends_where_the_reference_does(hip_backend, name, mode):
    import manta as m
    I = M.case_inputs(name)
    got = _run_fused(m, I, mode)
    want = _run_composed(m, I, mode)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s mode %d: the fused call is not its stages" % (name, mode)
    if name in FIXTURE:
        msg = M.same_as_fixture(GOLDEN, "end/%s/%d" % (name, mode), got)
        differ, _ = _velocity_check(name)
        print("end state %s mode %d: %s" % (name, mode, msg or "the reference's"))
        if differ == 0:
            assert msg is None, msg


def test_unknown_mode_moves_nothing(hip_backend):
    import manta as m
    I = M.case_inputs("self65")
    s = _solver(m)
    vp = _system(m, s, I["P"])
    mesh = s.create(m.Mesh)
    mesh.set_numpy(I["P"]["pos"])
    for call in (lambda: vp.advectSelf(integrationMode=3), lambda: vp.applyToMesh(mesh, integrationMode=-1)):
        with pytest.raises(RuntimeError, match="^unknown integration type$"):
            call()
    assert np.array_equal(vp.numpy()["pos"], I["P"]["pos"]) and np.array_equal(mesh.nodes_numpy()[0], I["P"]["pos"])
    from mantaflow_amd.core import _ptr
    with pytest.raises(RuntimeError, match="^unknown integration type$"):
        s.lib.call("mf_vortex_integrate", vp.np, vp.cap, _ptr(vp.pos), _ptr(vp.flag), M.PDELETE, vp.np, vp.cap, _ptr(vp.pos), _ptr(vp.flag), vp.vorticity.ptr,
                   vp.sigma.ptr, 1.0, 3, _ptr(vp._pos2), _ptr(vp._pos2), _ptr(vp._pos2), None, 0, s.stream)
    assert np.array_equal(vp.numpy()["pos"], I["P"]["pos"])


@pytest.mark.parametrize("name", list(M.DENSITY_CASES))
def test_density_from_levelset(hip_backend, name):
    import manta as m
    phi, value, sigma = M.density_inputs(name)
    sz, sy, sx = phi.shape
    s = _solver(m, (sx, sy, sz))
    g, d = s.create(m.LevelsetGrid), s.create(m.RealGrid)
    g.from_numpy(phi)
    d.from_numpy(np.full(phi.shape, np.nan, f32))
    m.densityFromLevelset(g, d, value=float(value), sigma=float(sigma))
    got = d.to_numpy()
    assert M.same_as_fixture(GOLDEN, "density/%s" % name, got) is None
    if sz == 1:
        assert not got.any()                                    # the k < 2 border test zeroes a 2-D grid, as in the reference


def _pkg_shape(m, s, shape):
    if shape[0] == "box":
        return m.Box(parent=s, p0=m.vec3(*shape[1]), p1=m.vec3(*shape[2]))
    return m.Sphere(parent=s, center=m.vec3(*shape[1]), radius=shape[2])


def test_loop_against_the_recorded_reference_run(hip_backend):
    """VPseedK41, advectSelf, advectInGrid with deletions per step and a compress() at the end: the channels follow"""
    import manta as m
    from mantaflow_amd import core
    C = M.LOOP
    core._seek_vortex_seed_stream(int(GOLDEN["loop/start"][0]))
    s = _solver(m, C["dims"], C["dt"])
    flags_np, vel_np = M.loop_grids()
    flags, vel = s.create(m.FlagGrid), s.create(m.MACGrid)
    flags.from_numpy(flags_np)
    vel.from_numpy(vel_np)
    vp = s.create(m.VortexParticleSystem)
    extra = vp.create(m.PdataReal)
    ball = _pkg_shape(m, s, C["shape"])
    sizes = []
    for _ in range(C["steps"]):
        m.VPseedK41(vp, ball, strength=C["strength"], sigma0=C["sigma0"], sigma1=C["sigma1"], probability=C["probability"], N=C["N"])
        _poison_pool(s)
        vp.advectSelf(scale=C["scale"], integrationMode=m.IntRK4)
        vp.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4, deleteInObstacle=True)
        sizes.append(vp.pySize())
    vp.compress()
    sizes.append(vp.pySize())
    print("loop sizes:", sizes)
    assert sizes == GOLDEN["loop/sizes"].tolist()
    got = vp.numpy()
    for ch in M.CHANNELS:
        msg = M.same_as_fixture(GOLDEN, "loop/" + ch, got[ch])
        assert msg is None, msg
    assert extra.size() == sizes[-1] and not extra.to_numpy().any()
    m.resetVortexSeedStream()


def test_calls_in_a_row_on_one_solver(hip_backend):
    """two systems and a mesh share one solver's pool; every call gives what it gives on a fresh solver"""
    import manta as m
    A, B, Mx = M.case_inputs("self257"), M.case_inputs("self65"), M.case_inputs("mesh257_600")
    alone = [_run_fused(m, A, 2), _run_fused(m, B, 1), _run_fused(m, Mx, 2), _run_fused(m, Mx, 0)]
    s = _solver(m)
    a, b, c = _system(m, s, A["P"]), _system(m, s, B["P"]), _system(m, s, Mx["P"])
    mesh = s.create(m.Mesh)
    k = lambda I: float(f32(I["scale"] / f32(DT)))
    a.advectSelf(scale=k(A))
    b.advectSelf(scale=k(B), integrationMode=m.IntRK2)
    mesh.set_numpy(Mx["nodes"], flags=Mx["nflags"])
    c.applyToMesh(mesh, scale=k(Mx))
    got = [a.numpy()["pos"], b.numpy()["pos"], mesh.nodes_numpy()[0]]
    mesh.set_numpy(Mx["nodes"], flags=Mx["nflags"])
    c.applyToMesh(mesh, scale=k(Mx), integrationMode=m.IntEuler)
    got.append(mesh.nodes_numpy()[0])
    for g, w in zip(got, alone):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


def test_empty_system_and_empty_mesh(hip_backend):
    import manta as m
    s = _solver(m)
    vp, mesh = s.create(m.VortexParticleSystem), s.create(m.Mesh)
    live = s._live
    for mode in M.MODES:
        vp.advectSelf(integrationMode=mode)
        vp.applyToMesh(mesh, integrationMode=mode)
    mesh.set_numpy(M.case_inputs("mesh65_257")["nodes"])
    before = mesh.nodes_numpy()[0]
    vp.applyToMesh(mesh)                                        # no sources: u = 0, x0 + 0
    assert np.array_equal(mesh.nodes_numpy()[0], before) and vp.pySize() == 0 and s._live == live
    full = _system(m, s, M.case_inputs("self65")["P"])
    full.applyToMesh(s.create(m.Mesh))                          # no targets
    assert np.array_equal(full.numpy()["pos"], M.case_inputs("self65")["P"]["pos"])
