"""CPU: the numpy model of the secondary particles (tests/secparts_model.py) held to the reference fixture
tests/golden/secparts.npz (tools/record_secparts.py wrote it from the reference's own plugin/secondaryparticles.cpp), and the
order-free statement of the sampling loop held to the literal serial loop.

Everything is bit for bit, except the positions and velocities of sampled particles: numpy's cos / sin are not glibc's cosf / sinf,
and each component must lie within 4 r 2^-23 + 3 ulp(reference value)."""
import os

import numpy as np
import pytest

import secparts_model as M

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "secparts.npz"))
f32 = np.float32


def bits_equal(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    d = got.view("u%d" % got.dtype.itemsize) != want.view("u%d" % got.dtype.itemsize)
    assert not d.any(), "%s: %d of %d words differ" % (tag, int(d.sum()), d.size)


def test_fixture_is_small_and_holds_outputs_only():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "secparts.npz")
    assert os.path.getsize(path) < 1 << 20
    assert not any(k.split("/")[-1] in ("vel_in", "phi", "potentials_in") for k in GOLDEN.files)


@pytest.mark.parametrize("name", sorted(M.POT_CASES))
def test_potentials(name):
    for k, v in M.run_pot_case(name).items():
        bits_equal(name + "/" + k, v, GOLDEN[name + "/" + k])


def test_potential_cases_hit_their_conditions():
    """the inputs' side of what the potential cases exist for"""
    I = M.pot_inputs("p3d_r1")
    raw = {}
    out = M.potentials(I["flags"], I["vel"], I["normal"], I["phi"], 1, *I["taus"], I["scale"], raw=raw)
    m = raw["cells"]
    assert (m & (raw["count"] == 0)).any() and np.isnan(out[3]).any()              # a fluid cell walled in: 0 / 0
    assert (m & (M._l2(raw["vi"]) == 0)).any()                                      # getNormalized of a zero velocity
    assert (m & (M._l2(raw["ni"]) == 1)).any()                                      # a unit normal: "normalized enough"
    for name, c in M.POT_CASES.items():
        fl = M.pot_inputs(name)["flags"][M._interior(c["dims"])]
        kinds = [(fl == t).mean() for t in (M.TypeObstacle, M.TypeOutflow, M.TypeInflow)]
        if fl.size >= 200:
            assert min(kinds) > 0.08, (name, kinds)         # about 15 % of each jtype kind
    I3 = M.pot_inputs("p3d_r3")
    assert (I3["dims"][0] - 6, I3["dims"][1] - 6, I3["dims"][2] - 6) == (3, 2, 1)
    with pytest.raises(AssertionError):
        M.potentials(I["flags"], I["vel"], I["normal"], I["phi"], 0, *I["taus"], I["scale"])


@pytest.mark.parametrize("mode", M.MODES)
def test_sampling(mode):
    stream = M.Stream()
    diff = {"pos": [0, 0], "ch0": [0, 0]}
    for name in M.SAMPLE_ORDER:
        key = "sample/%s/%s/" % (mode, name)
        assert stream.cursor == int(GOLDEN[key + "start"][0]), key          # the streams continue from case to case
        n0 = M.sample_inputs(name)["parts"].size()
        P, radii, sizes, used = M.run_sample_case(mode, name, stream)
        S = M.parts_state(P)
        assert np.array_equal(sizes, GOLDEN[key + "sizes"])
        for k in ("flag", "ch1", "ch2", "ch3"):
            bits_equal(key + k, S[k], GOLDEN[key + k])
        for k in ("pos", "ch0"):
            bits_equal(key + k + "[old]", S[k][:n0], GOLDEN[key + k][:n0])
            g, w = S[k][n0:], GOLDEN[key + k][n0:]
            if len(w):
                err = np.abs(g.astype(np.float64) - w.astype(np.float64))
                assert (err <= M.sample_bound(radii, w)).all(), (key, k, float((err / M.sample_bound(radii, w)).max()))
                diff[k][0] += int((g.view(np.uint32) != w.view(np.uint32)).any(axis=1).sum())
                diff[k][1] += len(w)
    print(mode, {k: "%d of %d not bit-identical" % tuple(v) for k, v in diff.items()})


def test_sampling_cases_hit_their_conditions():
    for mode in M.MODES:
        big = neg = ones = 0
        for name in M.SAMPLE_ORDER:
            I = M.sample_inputs(name)
            dt = I["dt"] if I["dt"] > 0 else I["solver_dt"]
            n = M.sample_entries(mode, I["flags"], I["potTA"], I["potWC"], I["potKE"], I["k_ta"], I["k_wc"], dt)["n"]
            big, neg, ones = max(big, int(n.max())), neg + int((n < 0).sum()), ones + int((n == 1).sum())
            if name == "s3d_none":
                assert not n.any()
            elif name != "s3d_twice":
                assert (n == 0).mean() > 0.8
        assert big > 300 and neg > 0 and ones > 0, (mode, big, neg, ones)
    I = M.sample_inputs("s3d")
    assert (I["parts"].flag & M.PDELETE).any() and len(I["parts"].channels) == 4


def _random_sampling_case(rng):
    dims = (int(rng.randint(3, 7)), int(rng.randint(3, 6)), int(rng.choice([1, 3, 4])))
    sh = M._shape(dims)
    on = rng.uniform(size=sh) < 0.35
    KE = np.where(on, rng.uniform(0, 1, sh), 0).astype(f32)
    TA, WC = rng.uniform(0, 1, sh).astype(f32), rng.uniform(0, 1, sh).astype(f32)
    flags = np.where(rng.uniform(size=sh) < 0.8, M.TypeFluid, M.TypeEmpty).astype(np.int32)
    vel = rng.uniform(-2, 2, sh + (3,)).astype(f32)
    if dims[2] == 1:
        vel[..., 2] = 0
    ratio = rng.uniform(0, 1, sh).astype(f32)
    return dict(flags=flags, vel=vel, potTA=TA, potWC=WC, potKE=KE, ratio=ratio, k_ta=float(rng.uniform(0, 8)), k_wc=float(rng.uniform(-6, 6)),
                dt=float(rng.choice([0.25, 0.5, 1.0])), start=int(rng.randint(0, 500)))


def test_orderfree_sampling_is_the_serial_loop():
    """about 1000 random small cases: the scan over per-entry counts and the bisection reproduce the running stream of the serial loop"""
    rng = np.random.RandomState(4242)
    emitted = negative = 0
    for q in range(1000):
        c = _random_sampling_case(rng)
        mode = M.MODES[q % 2]
        args = (mode, c["flags"], c["vel"], c["potTA"], c["potWC"], c["potKE"], c["ratio"], 1.0, 3.0, 0.3, 0.7, c["k_ta"], c["k_wc"], c["dt"])
        s1, s2 = M.Stream(c["start"]), M.Stream(c["start"])
        a, b = M.sample_serial(*args, s1), M.sample_orderfree(*args, s2)
        assert s1.cursor == s2.cursor and a["reals"] == b["reals"], q
        for k in ("pos", "vel", "life", "flag", "r"):
            bits_equal("case %d %s" % (q, k), a[k], b[k])
        emitted += len(a["flag"])
        negative += int((M.sample_entries(*args[:2], *args[3:6], c["k_ta"], c["k_wc"], c["dt"])["n"] < 0).sum())
    assert emitted > 5000 and negative > 100, (emitted, negative)


@pytest.mark.parametrize("name", sorted(n for n, c in M.UPDATE_CASES.items() if c.get("fixture", True)))
def test_update(name):
    for k, v in M.parts_state(M.run_update_case(name)).items():
        bits_equal(name + "/" + k, v, GOLDEN["update/%s/%s" % (name, k)])


def test_update_cases_hit_their_conditions():
    seen, cts, sizes = set(), set(), set()
    for name, c in M.UPDATE_CASES.items():
        I = M.update_inputs(name)
        info = {}
        P = M.run_update_case(name, info)
        sizes.add(c["n"])
        seen.add((c["mode"], bool(P.compresses), P.deletes > 0))
        cts |= set(int(v) for v in info["tunnel_ct"])
        # the preconditions (README, "Secondary particles"): no itype cell on the outermost layer; in cubic mode every foam or
        # bubble particle has an itype cell in reach
        assert not ((I["flags"] & I["itype"]) != 0)[~M._interior(I["dims"])].any(), name
        if c["mode"] == "cubic":
            assert (info["cubic_neighbours"] != 0).all(), name
        if c["n"] >= 1000 and not c.get("calm"):
            assert all((info["type"] == t).any() for t in (M.PSPRAY, M.PBUBBLE, M.PFOAM)) and info["dead"].any() and info["out"].any()
            fl = I["parts"].flag
            assert (fl & M.PTRACER).any() and (fl & M.PDELETE).any()
            x = I["parts"].pos
            assert ((x > -1) & (x < 0)).any()
    assert sizes == {1, 63, 64, 65, 1000, 5000}
    assert {1, 3} <= cts
    assert {("linear", True, False), ("linear", False, True), ("cubic", True, False), ("cubic", False, True)} <= seen


@pytest.mark.parametrize("name", sorted(M.DELETE_CASES))
def test_delete_in_obstacle(name):
    P = M.run_delete_case(name)
    for k, v in M.parts_state(P).items():
        bits_equal(name + "/" + k, v, GOLDEN["delete/%s/%s" % (name, k)])
    assert bool(P.compresses) == (name != "d3d_calm") and (P.deletes > 0) == (name == "d3d_calm")


@pytest.mark.parametrize("name", sorted(M.SET_CASES))
def test_set_from_levelset(name):
    I = M.set_inputs(name)
    bits_equal(name + "/flags", M.set_flags_from_levelset(I["flags"], I["phi"], I["exclude"], I["itype"]), GOLDEN["set/%s/flags" % name])
    bits_equal(name + "/vel", M.set_mac_from_levelset(I["vel"], I["phi"], I["c"]), GOLDEN["set/%s/vel" % name])


def test_loop_record_meets_its_conditions():
    c = GOLDEN["loop/counts"]
    assert c.shape == (M.LOOP["steps"], 6)
    assert 10 ** 3 <= c[:, 1].sum() <= 10 ** 5 and (c[:, 3:].max(axis=0) > 0).all()
    assert GOLDEN["loop/pots"].shape == (4,) + (M.LOOP["res"],) * 3
