"""GPU: the secondary-particle plugins through the package on the HIP backend, against the reference fixture
tests/golden/secparts.npz (how each array was produced: tools/record_secparts.py), against the numpy model on seeded inputs, and a
dam-break loop with a secondary system against a recorded reference run.

Everything is compared bit for bit, except the positions and velocities of newly sampled particles: there cos / sin of the azimuth
are the device's fp64 functions rounded once (the reference: glibc's cosf / sinf), and each component must lie within
4 r 2^-23 + 3 ulp(reference value) (secparts_model.sample_bound; DESIGN.md, "Secondary particles").  The share of new particles
that are not bit-identical is printed, not capped.  Outputs and pool scratch are pre-filled with NaN."""
import os

import numpy as np
import pytest

import nbflip_model as N
import secparts_model as M

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "secparts.npz"))
f32 = np.float32


def _solver(m, dims, dt=0.5):
    s = m.Solver(name="t", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)
    s.timestep = dt
    return s


def _grid(s, cls, arr):
    g = s.create(cls)
    g.from_numpy(arr)
    return g


def _nan_grid(s, cls, shape):
    return _grid(s, cls, np.full(shape, np.nan, f32))


def _poison_pool(s):
    """the next scratch grids the plugins take from the solver's pool hold NaN (garbage in the int grid)"""
    import torch
    for _ in range(2):
        s._pool.setdefault("vec", []).append(torch.full((3 * s.ncells,), float("nan"), dtype=torch.float32, device=s.device))
    s._pool.setdefault("int", []).append(torch.full((s.ncells,), 0x7fc00003, dtype=torch.int32, device=s.device))


def bits_equal(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    w = 4 if got.dtype.itemsize == 4 else 8
    d = got.view("u%d" % w) != want.view("u%d" % w)
    assert not d.any(), "%s: %d of %d words differ, first at %s" % (tag, int(d.sum()), d.size, np.argwhere(d)[0])


def dev_system(m, s, P):
    """the model's system [v_sec, l_sec, f_sec, extra int] on the device"""
    pp = s.create(m.BasicParticleSystem)
    pp.set_positions(P.pos, P.flag)
    pp.mDeletes, pp.mDeleteChunk = P.deletes, P.chunk
    chans = [pp.create({"vec3": m.PdataVec3, "real": m.PdataReal, "int": m.PdataInt}[c.kind]) for c in P.channels]
    for pd, c in zip(chans, P.channels):
        pd.from_numpy(c.data)
    return pp, chans


def dev_state(pp, chans):
    d = {"pos": pp.get_positions(), "flag": pp.get_flags()}
    for q, pd in enumerate(chans):
        d["ch%d" % q] = pd.to_numpy()
    return d


def check_state(tag, got, want, n0=None, radii=None, share=None):
    """bit for bit; with n0 / radii the positions and velocities of the particles from n0 on are held to the sampling bound"""
    assert set(got) == set(want)
    for k in sorted(want):
        if n0 is not None and k in ("pos", "ch0"):
            bits_equal(tag + "/" + k + "[old]", got[k][:n0], want[k][:n0])
            g, w = got[k][n0:], want[k][n0:]
            assert g.shape == w.shape, (tag, k, g.shape, w.shape)
            if len(w):
                err, bound = np.abs(g.astype(np.float64) - w.astype(np.float64)), M.sample_bound(radii, w)
                diff = (g.view(np.uint32) != w.view(np.uint32)).any(axis=1)
                print("%s/%s: %d new, %.3f %% not bit-identical, max error / bound %.3f" % (tag, k, len(w), 100.0 * diff.mean(), (err / bound).max()))
                if share is not None:
                    share.append((k, int(diff.sum()), len(w)))
                assert (err <= bound).all(), (tag, k, float((err / bound).max()))
        else:
            bits_equal(tag + "/" + k, got[k], want[k])


# ---------------------------------------------------------------------------------------------------------------------------------
# potentials
# ---------------------------------------------------------------------------------------------------------------------------------
def run_potentials(m, I):
    dims = I["dims"]
    sh = M._shape(dims)
    s = _solver(m, dims)
    outs = [_nan_grid(s, m.RealGrid, sh) for _ in range(4)]
    flags, vel, phi = _grid(s, m.FlagGrid, I["flags"]), _grid(s, m.MACGrid, I["vel"]), _grid(s, m.LevelsetGrid, I["phi"])
    normal = _grid(s, m.VecGrid, I["normal"])
    _poison_pool(s)
    m.flipComputeSecondaryParticlePotentials(outs[0], outs[1], outs[2], outs[3], flags, vel, normal, phi, I["radius"], *I["taus"], I["scale"],
                                             itype=I["itype"], jtype=I["jtype"])
    r = dict(zip(("potTA", "potWC", "potKE", "ratio"), (g.to_numpy() for g in outs)))
    r["normal"] = normal.to_numpy()
    return r


@pytest.mark.parametrize("name", sorted(M.POT_CASES))
def test_potentials_fixture(hip_backend, name):
    import manta as m
    got = run_potentials(m, M.pot_inputs(name))
    for k, v in got.items():
        bits_equal(name + "/" + k, v, GOLDEN[name + "/" + k])
    if name == "p3d_r1":
        assert np.isnan(got["ratio"]).any()          # the walled-in cell: 0 / 0


@pytest.mark.parametrize("name", ["p3d_r1", "p3d_r2", "p3d_row", "p2d_r2", "p2d_thin_r1", "p3d_types"])
def test_potentials_against_model(hip_backend, name):
    import manta as m
    I = M.pot_inputs(name, seed=9000 + M.POT_CASES[name]["seed"])
    got = run_potentials(m, I)
    want = dict(zip(("potTA", "potWC", "potKE", "ratio", "normal"),
                    M.potentials(I["flags"], I["vel"], I["normal"], I["phi"], I["radius"], *I["taus"], I["scale"], I["itype"], I["jtype"])))
    for k, v in got.items():
        bits_equal(name + "/" + k, v, want[k])


# ---------------------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------------------
def run_sample(m, mode, I, start):
    from mantaflow_amd import plugins
    dims = I["dims"]
    s = _solver(m, dims, I["solver_dt"])
    pp, chans = dev_system(m, s, I["parts"])
    g = {k: _grid(s, m.RealGrid, I[k]) for k in ("potTA", "potWC", "potKE", "ratio")}
    flags, vel = _grid(s, m.FlagGrid, I["flags"]), _grid(s, m.MACGrid, I["vel"])
    plugins._set_secondary_stream_cursor(mode, start)
    sizes = []
    for _ in range(I["calls"]):
        m.flipSampleSecondaryParticles(mode, flags, vel, pp, chans[0], chans[1], I["lMin"], I["lMax"], g["potTA"], g["potWC"], g["potKE"],
                                       g["ratio"], I["c_s"], I["c_b"], I["k_ta"], I["k_wc"], dt=I["dt"])
        sizes.append(pp.pySize())
    return dev_state(pp, chans), np.array(sizes, np.int64), plugins.flipSampleSecondaryParticlesStats["cursor"], pp


@pytest.mark.parametrize("mode", M.MODES)
def test_sampling_fixture(hip_backend, mode):
    """every sampling case of the mode, each started at the stream offset the recorder stored; the next case's offset is where
    this one must end"""
    import manta as m
    share = []
    for q, name in enumerate(M.SAMPLE_ORDER):
        key = "sample/%s/%s/" % (mode, name)
        I = M.sample_inputs(name)
        n0 = I["parts"].size()
        start = int(GOLDEN[key + "start"][0])
        got, sizes, cursor, pp = run_sample(m, mode, I, start)
        assert np.array_equal(sizes, GOLDEN[key + "sizes"]), (key, sizes, GOLDEN[key + "sizes"])
        P, radii, _, used = M.run_sample_case(mode, name, M.Stream(start))
        assert cursor == start + used
        if q + 1 < len(M.SAMPLE_ORDER):
            assert cursor == int(GOLDEN["sample/%s/%s/start" % (mode, M.SAMPLE_ORDER[q + 1])][0])
        want = {k: GOLDEN[key + k] for k in ("pos", "flag", "ch0", "ch1", "ch2", "ch3")}
        check_state(key + "reference", got, want, n0, radii, share)
        check_state(key + "model", got, M.parts_state(P), n0, radii)
        if sizes[-1] > n0:
            assert pp.mDeleteChunk == sizes[-1] // 20
        # the extra channels: zero on the new entries, untouched on the old ones
        assert (got["ch3"][n0:] == 0).all() and (got["ch2"][n0:] == 0).all()
        bits_equal(key + "old extra", got["ch3"][:n0], I["parts"].channels[3].data)
    for k in ("pos", "ch0"):
        d, n = sum(a for kk, a, _ in share if kk == k), sum(b for kk, _, b in share if kk == k)
        print("sampling %s, %s: %d of %d new particles not bit-identical to the reference (%.2f %%)" % (mode, k, d, n, 100.0 * d / max(n, 1)))


@pytest.mark.parametrize("mode", M.MODES)
def test_sampling_nothing_to_emit(hip_backend, mode):
    import manta as m
    I = M.sample_inputs("s3d_none")
    got, sizes, cursor, _ = run_sample(m, mode, I, 17)
    assert cursor == 17 and sizes[-1] == I["parts"].size()
    check_state("none", got, M.parts_state(I["parts"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# update, flipDeleteParticlesInObstacle
# ---------------------------------------------------------------------------------------------------------------------------------
def run_update(m, I):
    s = _solver(m, I["dims"], I["solver_dt"])
    pp, chans = dev_system(m, s, I["parts"])
    flags, vel, ratio = _grid(s, m.FlagGrid, I["flags"]), _grid(s, m.MACGrid, I["vel"]), _grid(s, m.RealGrid, I["ratio"])
    m.flipUpdateSecondaryParticles(I["mode"], pp, chans[0], chans[1], chans[2], flags, vel, ratio, I["radius"], I["gravity"], I["k_b"], I["k_d"],
                                   I["c_s"], I["c_b"], dt=I["dt"], scale=I["scale"], exclude=I["exclude"], antitunneling=I["at"],
                                   itype=I["itype"])
    return dev_state(pp, chans), pp


@pytest.mark.parametrize("name", sorted(M.UPDATE_CASES))
def test_update(hip_backend, name):
    import manta as m
    I = M.update_inputs(name)
    n0 = I["parts"].size()
    got, pp = run_update(m, I)
    P = M.run_update_case(name)
    check_state(name + "/model", got, M.parts_state(P))
    assert (pp.mDeletes, pp.mDeleteChunk) == (P.deletes, P.chunk)
    print(name, "particles", n0, "->", pp.pySize(), "compressed" if P.compresses else "kills left in place: %d" % P.deletes)
    if M.UPDATE_CASES[name].get("fixture", True):
        check_state(name + "/reference", got, {k: GOLDEN["update/%s/%s" % (name, k)] for k in got})


@pytest.mark.parametrize("name", sorted(M.DELETE_CASES))
def test_delete_in_obstacle(hip_backend, name):
    import manta as m
    I = M.update_inputs(name, M.DELETE_CASES)
    s = _solver(m, I["dims"])
    pp, chans = dev_system(m, s, I["parts"])
    m.flipDeleteParticlesInObstacle(pp, _grid(s, m.FlagGrid, I["flags"]))
    got = dev_state(pp, chans)
    P = M.run_delete_case(name)
    check_state(name + "/model", got, M.parts_state(P))
    check_state(name + "/reference", got, {k: GOLDEN["delete/%s/%s" % (name, k)] for k in got})
    assert (pp.mDeletes, pp.mDeleteChunk) == (P.deletes, P.chunk)


@pytest.mark.parametrize("name", sorted(M.SET_CASES))
def test_set_from_levelset(hip_backend, name):
    import manta as m
    I = M.set_inputs(name)
    s = _solver(m, I["dims"])
    flags, phi, vel = _grid(s, m.FlagGrid, I["flags"]), _grid(s, m.RealGrid, I["phi"]), _grid(s, m.MACGrid, I["vel"])
    m.setFlagsFromLevelset(flags, phi, exclude=I["exclude"], itype=I["itype"])
    m.setMACFromLevelset(vel, phi, I["c"])
    bits_equal(name + "/flags", flags.to_numpy(), GOLDEN["set/%s/flags" % name])
    bits_equal(name + "/vel", vel.to_numpy(), GOLDEN["set/%s/vel" % name])
    bits_equal(name + "/flags model", flags.to_numpy(), M.set_flags_from_levelset(I["flags"], I["phi"], I["exclude"], I["itype"]))
    bits_equal(name + "/vel model", vel.to_numpy(), M.set_mac_from_levelset(I["vel"], I["phi"], I["c"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------------
def test_loop_call_by_call_and_end_to_end(hip_backend):
    """the recorded dam break: before each of the four secondary-particle calls the device state goes to the model and the call's
    result is compared with the model's; the per-step counts and the final potentials are compared with the reference run"""
    import manta as m
    from mantaflow_amd import plugins
    C = M.LOOP
    plugins._set_secondary_stream_cursor("single", int(GOLDEN["loop/start"][0]))
    held = {}
    share = []

    def model_parts(O):
        return N.model_from_device(O["sec"], O["chans"], [(None, False)] * 3)

    def before(call, t, O):
        O["s"].sync()
        held["grids"] = {k: O[k].to_numpy() for k in ("flags", "vel", "phi", "normal", "potTA", "potWC", "potKE", "ratio")}
        held["parts"] = model_parts(O)
        held["cursor"] = plugins._secondary_stream("single").cursor

    def after(call, t, O):
        G, P = held["grids"], held["parts"]
        tag = "step %d %s" % (t, call)
        if call == "potentials":
            want = M.potentials(G["flags"], G["vel"], G["normal"], G["phi"], C["radius"], *C["taus"], C["scale"])
            for k, w in zip(("potTA", "potWC", "potKE", "ratio", "normal"), want):
                bits_equal(tag + "/" + k, O[k].to_numpy(), w)
            return
        n0, radii = None, None
        if call == "sample":
            stream = M.Stream(held["cursor"])
            new = M.sample_orderfree("single", G["flags"], G["vel"], G["potTA"], G["potWC"], G["potKE"], G["ratio"], C["lMin"], C["lMax"], C["c_s"],
                                     C["c_b"], C["k_ta"], C["k_wc"], C["dt"], stream)
            n0, radii = P.size(), new["r"]
            M.sample(P, 0, 1, new)
            assert plugins._secondary_stream("single").cursor == stream.cursor, tag
        elif call == "update":
            M.update("linear", P, 0, 1, 2, G["flags"], G["vel"], G["ratio"], 1, C["gravity"], C["k_b"], C["k_d"], C["c_s"], C["c_b"], C["dt"],
                     1.0 / C["res"], M.PTRACER, C["antitunneling"])
        else:
            M.delete_in_obstacle(P, G["flags"])
        got = dev_state(O["sec"], O["chans"])
        want = {k: v for k, v in M.parts_state(P).items()}
        check_state(tag, got, want, n0, radii, share if call == "sample" else None)
        assert (O["sec"].mDeletes, O["sec"].mDeleteChunk) == (P.deletes, P.chunk), tag

    counts, pots = M.sec_loop(m, before, after)
    print("loop counts (live, spawned, slots, spray, bubble, foam):\n", counts)
    for k in ("pos", "ch0"):
        d, n = sum(a for kk, a, _ in share if kk == k), sum(b for kk, _, b in share if kk == k)
        print("loop, %s: %d of %d sampled particles not bit-identical to the model" % (k, d, n))
    assert np.array_equal(counts, GOLDEN["loop/counts"]), np.argwhere(counts != GOLDEN["loop/counts"])[:4]
    bits_equal("loop/pots", pots, GOLDEN["loop/pots"])
    assert 10 ** 3 <= counts[:, 1].sum() <= 10 ** 5 and (counts[:, 3:].max(axis=0) > 0).all()
