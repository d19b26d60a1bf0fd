"""CPU: the numpy model of the mesh connectivity tables, smoothMesh and killSmallComponents (tests/meshops_model.py) against the
reference's recorded outputs (tests/golden/meshops.npz) on every case, its order-free forms against the literal serial loops on seeded
random meshes and masks, and the derived bound between two summation orders of the volume terms."""
import numpy as np
import pytest

import meshops_model as M

GOLDEN = np.load(M.GOLDEN)
i32 = np.int32


def _same(key, a):
    msg = M.same_as_fixture(GOLDEN, key, a)
    assert msg is None, msg


@pytest.mark.parametrize("name", sorted(M.CONNECTIVITY_CASES))
def test_connectivity_model_equals_the_fixture_and_the_literal_loops(name):
    m = M.CONNECTIVITY_CASES[name]()
    c = M.connectivity("test", m)
    for k in ("opposite", "nodeOff", "nodes", "triOff", "tris"):
        _same("conn/%s/%s" % (name, k), c[k])
    if m["tris"].shape[0] <= 700:                      # the literal search is quadratic
        assert np.array_equal(c["opposite"], M.corners_literal(m["tris"]))
    for a, b in zip(M.ring_literal(m["tris"], m["pos"].shape[0]), (c["nodeOff"], c["nodes"], c["triOff"], c["tris"])):
        assert np.array_equal(a, b) and a.dtype == b.dtype


def test_the_cases_are_what_they_exist_for():
    count = lambda name: M.corners(M.CONNECTIVITY_CASES[name]()["tris"])[1:]
    assert count("book3") == (0, 7) and count("book4") == (0, 1) and count("sphere17") == (0, 0)
    for n in (3, 61, 62, 63, 300):
        m = M.bipyramid(n)
        c = M.connectivity("test", m)
        assert m["pos"].shape[0] == n + 2 and m["tris"].shape[0] == 2 * n and np.diff(c["nodeOff"])[n:].tolist() == [n, n]
    t = M.CONNECTIVITY_CASES["perm_bipyr63"]()["tris"]
    assert (np.diff(t.reshape(-1)) < 0).any()
    # the group rule on a group of three and of four: c_i -> c_{i+1}, the last one back to its predecessor
    opp = M.corners(M.book4()["tris"])[0]
    g = [c for c in range(24) if set(np.roll(M.book4()["tris"][c // 3], -(c % 3))[1:].tolist()) == {0, 1}]
    assert len(g) == 4 and [opp[c] for c in g] == [g[1], g[2], g[3], g[2]]


@pytest.mark.parametrize("name", sorted(M.REFUSED_CASES))
def test_refused_connectivity(name):
    make, msg = M.REFUSED_CASES[name]
    with pytest.raises(RuntimeError) as e:
        M.connectivity("who", make())
    assert str(e.value) == (msg % "who" if "%s" in msg else msg)
    assert name == "repeated" or str(e.value) == GOLDEN["msg/" + name].tobytes().decode()       # the reference's own text where it has one
    if name != "repeated":
        with pytest.raises(RuntimeError, match="can't rebuild corners"):
            M.corners_literal(make()["tris"])


def test_order_free_corner_rule_equals_the_literal_search_on_random_triangle_soups():
    r = np.random.RandomState(11)
    seen_multi = 0
    for q in range(300):
        n, T = r.randint(3, 9), r.randint(1, 14)
        tris = np.array([r.choice(n, 3, replace=False) for _ in range(T)], i32)
        opp, singles, multi = M.corners(tris)
        seen_multi += multi > 0
        if singles:
            with pytest.raises(RuntimeError):
                M.corners_literal(tris)
        else:
            assert np.array_equal(opp, M.corners_literal(tris)), q
        for a, b in zip(M.ring_literal(tris, n), M.ring(tris, n)):
            assert np.array_equal(a, b)
    assert seen_multi > 50


@pytest.mark.parametrize("name", sorted(M.SMOOTH_CASES))
def test_smooth_model_equals_the_fixture(name):
    m, dt, strength, steps, minLength = M.SMOOTH_CASES[name]()
    out, sums = M.smooth_mesh(m, dt, strength, steps, minLength)
    _same("smooth/%s/pos" % name, out["pos"])
    _same("smooth/%s/sums" % name, sums)
    for k in ("normal", "flags", "tris", "tflags"):
        assert np.array_equal(out[k], m[k])
    if m["tris"].shape[0] <= 700:
        lit, _ = M.smooth_mesh(m, dt, strength, steps, minLength, literal=True)
        assert lit["pos"].tobytes() == out["pos"].tobytes()
    fixed = (m["flags"] & 1) != 0
    assert out["pos"][fixed].tobytes() == m["pos"][fixed].tobytes()


def test_smooth_cases_are_what_they_exist_for():
    m, dt, strength, steps, ml = M.SMOOTH_CASES["clamp"]()
    assert np.float32(dt) * np.float32(strength) > 1
    m, *_ = M.SMOOTH_CASES["isolated"]()
    out, _ = M.smooth_mesh(m, 0.5, 0.6)
    assert m["flags"][-1] == 1 and out["pos"][-1].tobytes() == m["pos"][-1].tobytes()           # fixed and isolated: stays
    one, _ = M.smooth_mesh(m, 0.5, 0.6, sums=(np.array([1., 0, 0, 0]), np.array([1., 0, 0, 0])))
    assert (one["pos"][-2] == 0).all()                                                          # isolated, not fixed: the origin
    m, *_ = M.SMOOTH_CASES["coincident"]()
    c = M.connectivity("t", m)
    temp = M.smooth_step(m["pos"], c["nodeOff"], c["nodes"], c["triOff"], np.float32(0.3), np.float32(1e-5))
    moved = (temp != m["pos"]).any(1)
    assert not moved[0] and not moved[1] and moved[2:].all()
    m, dt, strength, steps, ml = M.SMOOTH_CASES["minlength"]()
    c = M.connectivity("t", m)
    assert (M.smooth_step(m["pos"], c["nodeOff"], c["nodes"], c["triOff"], np.float32(0.3), np.float32(ml)) == m["pos"]).all()


def test_sum_bound_holds_between_the_serial_and_a_pairwise_sum():
    for name in ("sphere17", "apex300", "two"):
        m = M.SMOOTH_CASES[name]()[0]
        terms = M.volume_terms(m["pos"], m["tris"])
        a, b = M.serial_sums(terms), M.pairwise_sums(terms)
        assert (np.abs(a - b) <= M.sum_bound(terms)).all(), name
        assert a.tobytes() == np.cumsum(terms, 0)[-1].tobytes()             # the serial order, twice
    assert (M.sum_bound(np.ones((1, 4))) == 0).all()


@pytest.mark.parametrize("name", sorted(M.KILL_CASES))
def test_kill_model_equals_the_fixture_and_the_literal_loops(name, capsys):
    m, elements = M.KILL_CASES[name]()
    out, stats = M.kill_small_components(m, elements)
    msg = M.mesh_same_as_fixture(GOLDEN, "kill/" + name, out)
    assert msg is None, msg
    assert GOLDEN["kill/%s/message" % name].tobytes().decode() == (M.kill_message(stats) if stats["tris"] else "")
    lit, lstats = M.kill_small_components(m, elements, literal=True)
    assert lstats == stats
    for k in M.MESH_KEYS:
        assert lit[k].tobytes() == out[k].tobytes(), k


def test_kill_cases_are_what_they_exist_for():
    stats = {name: M.kill_small_components(*make())[1] for name, make in M.KILL_CASES.items()}
    assert stats["equal"]["tris"] == 0 and stats["plus1"]["tris"] == 8 and stats["none_default"]["tris"] == 0
    assert stats["all"]["tris"] == 38 and stats["default"]["tris"] == 16 and stats["sphere17"]["tris"] == 4
    m, el = M.KILL_CASES["chained"]()
    c = M.connectivity("t", m)
    taint, _ = M.taint_mask(c["opposite"], 12, el)
    assert np.nonzero(taint)[0].tolist() == [1, 2, 5, 9] and M.tri_sources(taint).tolist() == [0, 8, 11, 3, 4, 10, 6, 7]
    assert M.tri_sources(np.isin(np.arange(10), [7, 2, 1])).tolist() == [0, 9, 8, 3, 4, 5, 6]     # slot 2 <- old 8, slot 1 <- old 9
    for name in ("interleaved", "shuffled", "isolated"):
        m, el = M.KILL_CASES[name]()
        c = M.connectivity("t", m)
        d = M.deleted_nodes(m["tris"], M.taint_mask(c["opposite"], m["tris"].shape[0], el)[0], m["pos"].shape[0])
        assert d != sorted(d) and min(d) < m["pos"].shape[0] - len(d) <= max(d), name


@pytest.mark.parametrize("name", sorted(M.KILL_REFUSED))
def test_kill_refusals(name):
    make, msg = M.KILL_REFUSED[name]
    with pytest.raises(RuntimeError) as e:
        M.kill_small_components(*make())
    assert str(e.value) == msg


def test_order_free_removal_equals_the_literal_loops_on_random_masks():
    r = np.random.RandomState(5)
    for q in range(1500):
        T = r.randint(1, 40)
        taint = r.uniform(size=T) < r.choice([0.1, 0.5, 0.9])
        tris = np.arange(3 * T, dtype=i32).reshape(T, 3)
        fl = np.arange(T, dtype=i32) + 100
        want = M.remove_tris_literal(tris, fl, taint)
        src = M.tri_sources(taint)
        assert np.array_equal(tris[src], want[0]) and np.array_equal(fl[src], want[1]), q
        n = r.randint(1, 30)
        deleted = r.permutation(n)[:r.randint(0, n + 1)].tolist()
        assert M.new_index(deleted, n) == M.new_index_literal(deleted, n), q


def test_order_free_components_and_deleted_nodes_equal_the_literal_walks_on_random_meshes():
    r = np.random.RandomState(6)
    for q in range(1000):
        parts = [M.bipyramid(r.randint(3, 7), q) if r.uniform() < 0.6 else M.tetrahedron(q) for _ in range(r.randint(1, 5))]
        m = M.join(parts, seed=q, tri_seed=q + 1)
        T, n = m["tris"].shape[0], m["pos"].shape[0]
        opp = M.corners(m["tris"])[0]
        el = r.randint(3, 14)
        a, na = M.taint_mask(opp, T, el)
        b, nb = M.taint_mask(opp, T, el, literal=True)
        assert np.array_equal(a, b) and na == nb == len(parts), q
        assert M.deleted_nodes(m["tris"], a, n) == M.deleted_nodes_literal(m["tris"], a, n), q
