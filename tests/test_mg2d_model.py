"""tests/mg2d_model.py, the numpy statement of the reference's GridMg in its 2-D mode, against tests/golden/mg2d.npz (recorded from
the reference by tools/record_mg2d.py): every recorded array of every stage system bit for bit; the size table; the literal serial
colour sweep against the vectorised one on random small systems; the level-1 path list's count, sc range and sort keys against the
reference's recorded list.  No GPU, no reference build."""
import numpy as np
import pytest

import mg2d_cases as C
import mg2d_model as M
import mg_model as M3


@pytest.fixture(scope="module")
def golden():
    return np.load(C.GOLDEN)


def test_size_table():
    for dims, levels in C.SHAPES + [(C.FRACTIONS_DIMS, C.FRACTIONS_LEVELS)]:
        got = M.level_sizes(dims)
        assert got == levels == M3.level_sizes(dims), (dims, got)
        for fine, coarse in zip(got, got[1:]):
            assert coarse == ((fine[0] + 2) // 2, (fine[1] + 2) // 2, 1)
            assert not (fine[0] <= 5 and fine[1] <= 5) and fine[0] * fine[1] > 1000
        last = got[-1]
        assert (last[0] <= 5 and last[1] <= 5) or last[0] * last[1] <= 1000
        assert last[0] * last[1] <= 1000      # one thread per vertex in the 1024-thread tail
    # what the table is there for
    assert C.LEVELS[(40, 25, 1)] == [(40, 25, 1)] and C.LEVELS[(78, 48, 1)][-1] == (40, 25, 1)
    assert 90 * 91 <= C.TAIL_VERTS < 91 * 91 and 129 * 66 > C.TAIL_VERTS
    assert [C.expected_tail_first(C.LEVELS[d]) for d in ((90, 91, 1), (91, 91, 1), (257, 130, 1), (30, 30, 1))] == [0, 1, 2, 0]


@pytest.mark.parametrize("tag", C.stage_tags())
def test_model_equals_fixture(golden, tag):
    """types, operator, b and x of every level after setA and one V-cycle: the model has the reference's bits"""
    dims, A, rhs = C.stage_system(tag)
    H = C.model_hierarchy(golden, tag, dims, A)
    cyc = M.vcycle(H, rhs)
    nl = int(golden[tag + "__levels"])
    assert H.nl == nl and H.sizes == [tuple(int(v) for v in golden[tag + "__size%d" % l]) for l in range(nl)]
    for l in range(nl):
        a = H.A2[l].copy()
        a[:, H.t[l] == 0] = 0
        for key, got in (("type", H.t[l]), ("A", a), ("b", cyc["b"][l]), ("x", cyc["x"][l])):
            bad = C.recorded_mismatch(golden, "%s__%s%d" % (tag, key, l), got)
            assert bad is None, bad
    if tag.endswith("__lap") and nl > 1:
        assert H.A1_owned.all()      # integer system: every order of the level-1 sums gives the same bits


def _random_hierarchy(dims, seed):
    """an integer Laplace system with random obstacles and a few non-integer diagonals above level 0's reach (the rows stay
    diagonally dominant), so that the sweeps see inactive vertices, borders and both parities"""
    import cases
    import util
    flags = util.make_flags(*dims, seed=seed, obstacles=True, empty_top=seed % 2 == 0)
    A = C.planes3(cases.run_laplace_impl(util.Impl("oracle"), dims, flags, None))
    return M.setup(dims, A)


@pytest.mark.parametrize("dims,seed", [((9, 8, 1), 3), ((12, 7, 1), 4), ((37, 29, 1), 5), ((36, 30, 1), 6)], ids=str)
def test_serial_sweep_equals_vectorised(dims, seed):
    """knSmoothColor one vertex at a time in the reference's block / offset order, in place, against the vectorised colour pass of the
    model, forwards and backwards, on every level"""
    H = _random_hierarchy(dims, seed)
    rng = np.random.default_rng(seed)
    assert H.nl == (2 if dims[0] > 30 else 1)
    for l in range(H.nl):
        n = H.sizes[l][0] * H.sizes[l][1]
        x = rng.uniform(-1, 1, n).astype(np.float32)
        b = rng.uniform(-1, 1, n).astype(np.float32)
        for reverse in (False, True):
            want = M.smooth_serial(H, l, x, b, reverse)
            got = M3.smooth(H, l, x.copy(), b, reverse)
            assert got.tobytes() == want.tobytes(), (dims, l, reverse)
            assert (got != x)[H.t[l] != 0].any() and (got == x)[H.t[l] == 0].all()


def test_path_list(golden):
    """the generation order of multigrid.cpp:292-312 with mDim = 2: the reference's count, sc in 0..4, and, sorted stably by the
    reference's comparator, the recorded list up to the order inside the groups the comparator ties (which belongs to std::sort
    and is checked against the library's own list by tools/mg2d_host_check.py)"""
    rec = golden["paths"]
    mine = M.paths_unsorted()
    assert len(mine) == rec.shape[0] and not rec[:, 11].any()
    assert sorted({p[6] for p in mine}) == [0, 1, 2, 3, 4] == sorted(set(rec[:, 6].tolist()))
    assert {p[7] for p in mine} == {0, 1, 2}

    def row(p):
        return tuple(p[:9]) + (int(np.float32(p[9]).view(np.int32)), int(np.float32(p[10]).view(np.int32)))

    rec_rows = [tuple(int(v) for v in r[:11]) for r in rec]
    assert sorted(row(p) for p in mine) == sorted(rec_rows)
    keys = [(r[6], (r[2] + 1) + 3 * (r[3] + 1)) for r in rec_rows]
    assert keys == sorted(keys) == [M.path_sort_key(p) for p in sorted(mine, key=M.path_sort_key)]
    # the comparator does leave ties: the order of the terms inside one stencil entry is the sort's
    assert len(set(keys)) < len(keys)
