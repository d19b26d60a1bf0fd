"""The numpy model of the multigrid hierarchy (tests/mg_model.py) against the two recordings of the reference's GridMg, bit for
bit, without a GPU and without the compiled reference:
  tests/golden/multigrid_levels.npz  (tools/record_mg_levels.py): per edge case and stage system the types, the operator, and b and
                                     x of every level after one V-cycle -- as arrays, or as SHA-256 digests above 4096 elements
  tests/golden/multigrid.npz         the stage__ entries, recorded independently: types per level, A1, the coarsest operator and
                                     the V-cycle's result
and against itself: the bucket-heap selection against a literal "scan for the minimum" statement of the same rule, the level
table of mg_cases.EDGE_SHAPES against the size rule."""
import os

import numpy as np
import pytest

import mg_cases
import mg_model as M


@pytest.fixture(scope="module")
def levels():
    return np.load(mg_cases.LEVELS_GOLDEN)


@pytest.mark.parametrize("tag", mg_cases.edge_stage_tags())
def test_model_reproduces_levels_fixture(levels, tag):
    dims, A, rhs = mg_cases.edge_stage_system(tag)
    H = mg_cases.model_hierarchy(levels, tag, dims, A)
    cyc = M.vcycle(H, rhs)
    assert int(levels[tag + "__levels"]) == H.nl
    for l in range(H.nl):
        assert tuple(int(v) for v in levels[tag + "__size%d" % l]) == H.sizes[l]
        op = H.A[l].copy()
        op[:, H.t[l] == 0] = 0
        for what, got in (("type", H.t[l]), ("A", op), ("b", cyc["b"][l]), ("x", cyc["x"][l])):
            bad = mg_cases.recorded_mismatch(levels, "%s__%s%d" % (tag, what, l), got)
            assert bad is None, bad
    if tag.endswith("__lap") and H.nl > 1:
        assert H.A1_owned.all(), "an integer system whose level-1 sums depend on their order"


@pytest.mark.parametrize("kind", list(mg_cases.STAGE_CASES))
def test_model_reproduces_stage_entries_of_multigrid_npz(kind):
    g = np.load(mg_cases.GOLDEN)
    dims = mg_cases.STAGE_CASES[kind]
    name = mg_cases.case_name(kind, dims)
    flags, A, rhs = mg_cases.stage_inputs(kind, dims)
    H = M.setup(dims, A)
    assert int(g["stage__%s__levels" % name]) == H.nl
    checked = 0
    for l in range(H.nl):
        assert tuple(int(v) for v in g["stage__%s__size%d" % (name, l)]) == H.sizes[l]
        assert np.array_equal(g["stage__%s__type%d" % (name, l)], H.t[l]), "vertex types of level %d" % l
        key = "stage__%s__A%d" % (name, l)
        if key in g.files:
            op = H.A[l].copy()
            op[:, H.t[l] == 0] = 0
            assert op.tobytes() == g[key].tobytes(), "operator of level %d" % l
            checked += 1
    assert checked == 2      # A1 and the coarsest operator
    assert M.vcycle(H, rhs)["result"].tobytes() == g["stage__%s__vcycle" % name].tobytes()


class ScanHeap(object):
    """the rule of the reference's heap said literally: among the IDs with the smallest key, the one whose key was set last"""

    def __init__(self, n, k):
        self.key, self.stamp, self.clock = {}, {}, 0

    @property
    def size(self):
        return len(self.key)

    def get_key(self, i):
        return self.key.get(i, -1)

    def set_key(self, i, k):
        if self.get_key(i) == k:
            return
        self.key.pop(i, None)
        if k != -1:
            self.clock += 1
            self.key[i], self.stamp[i] = k, self.clock

    def pop_min(self):
        kmin = min(self.key.values())
        i = max((j for j, k in self.key.items() if k == kmin), key=lambda j: self.stamp[j])
        del self.key[i]
        return i


def test_heap_selection_equals_scan_for_minimum():
    rng = np.random.default_rng(11)
    seen_inactive_coarse = 0
    for trial in range(300):
        fsize = tuple(int(s) for s in rng.integers(1, 8, 3))
        csize = tuple((s + 2) // 2 for s in fsize)
        tf = (rng.random(fsize[0] * fsize[1] * fsize[2]) < rng.choice([0.3, 0.7, 0.95, 1.0])).astype(np.uint8)
        a = M.select_coarse(fsize, tf, csize)
        b = M.select_coarse(fsize, tf, csize, heap_cls=ScanHeap)
        assert np.array_equal(a, b), (trial, fsize)
        # every active fine vertex interpolates from at least one active coarse vertex
        X, Y, Z = M._coords(fsize)
        for v in np.nonzero(tf)[0]:
            got = [a[ix + csize[0] * (iy + csize[1] * iz)] for iz in range(Z[v] // 2, (Z[v] + 1) // 2 + 1) for iy in range(Y[v] // 2, (Y[v] + 1) // 2 + 1)
                   for ix in range(X[v] // 2, (X[v] + 1) // 2 + 1)]
            assert any(got), (trial, fsize, v)
        seen_inactive_coarse += int((a == 0).sum())
    assert seen_inactive_coarse > 300


def test_level_table_follows_the_size_rule():
    assert len(mg_cases.EDGE_SHAPES) == 15 and len(mg_cases.EDGE_CASES) == 58
    for dims, want in mg_cases.EDGE_SHAPES:
        assert M.level_sizes(dims) == want, dims
        sx, sy, sz = want[-1]
        assert sx * sy * sz <= 1000 or max(sx, sy, sz) <= 5
    one = [d for d, lv in mg_cases.EDGE_SHAPES if len(lv) == 1]
    assert one == [(10, 10, 10), (5, 5, 5), (6, 5, 5)]
    assert 32 * 16 * 16 == 8192 and mg_cases.EDGE_LEVELS[(18, 18, 18)][-1] == (10, 10, 10)
    skipped = [(k, d) for d, _ in mg_cases.EDGE_SHAPES for k in mg_cases.KINDS if (k, d) not in mg_cases.EDGE_CASES]
    assert skipped == [("liq", (3, 3, 120)), ("liq", (120, 3, 3))]
    # the sizes of the existing solve table all have more than one level
    assert all(len(M.level_sizes(d)) > 1 for d in mg_cases.SIZES)


def test_levels_fixture_is_small_and_complete(levels):
    assert os.path.getsize(mg_cases.LEVELS_GOLDEN) < (1 << 20)
    want = set()
    for tag in mg_cases.edge_stage_tags():
        dims = tuple(int(s) for s in tag.split("__")[0].split("_")[1].split("x"))
        sizes = M.level_sizes(dims)
        assert int(levels[tag + "__levels"]) == len(sizes)
        want.add(tag + "__levels")
        for l, s in enumerate(sizes):
            want.add(tag + "__size%d" % l)
            n = s[0] * s[1] * s[2]
            for what, size in (("type", n), ("A", n * (4 if l == 0 else 14)), ("b", n), ("x", n)):
                want.add("%s__%s%d%s" % (tag, what, l, "__sha" if size > 4096 else ""))
        if tag.endswith("__coef") and len(sizes) > 1:
            want |= {tag + "__A1fix_idx", tag + "__A1fix_val"}
    for kind, dims in mg_cases.EDGE_CASES:
        name = mg_cases.case_name(kind, dims)
        want |= {name + "__iters", name + "__sha_p", name + "__sha_v"}
        assert 0 < int(levels[name + "__iters"]) < 100
    assert set(levels.files) == want
    for k in levels.files:
        assert levels[k].size <= 4096 and (not k.endswith("__sha") and "__sha_" not in k or levels[k].shape == (32,)), k
