"""-m gpu: the multigrid hierarchy of the HIP library (mantaflow_amd/csrc/multigrid.hip) level by level, at shapes no solve of
tests/test_gpu_multigrid.py reaches (mg_cases.EDGE_SHAPES: one-level hierarchies, thin and lopsided levels, level 0 on either
side of the 8192-vertex hand-over between the grid-wide kernels and the single-workgroup tail, a coarsest level of exactly 1000
vertices), bit for bit against
  tests/golden/multigrid_levels.npz   the reference's GridMg as tools/record_mg_levels.py recorded it: types, operators, and b
                                      and x of EVERY level after one V-cycle
  tests/mg_model.py                   the numpy statement of the same, which tests/test_mg_model.py ties to that file and to the
                                      stage__ entries of multigrid.npz
  oracle/_ref/libmanta_ref.so         for the solves
All through the C ABI of include/manta_hip_multigrid.h (mf_mg_create / set_a / vcycle / info / read_level).  There is no
tolerance anywhere: the contract of this family is "bit-identical to the reference's"."""
import ctypes

import numpy as np
import pytest

import cases
import mg_cases
import mg_model as M
import util
from mg_cases import PcMGDynamic, PcMGStatic
from util import assert_bitexact

pytestmark = pytest.mark.gpu

TAIL_VERTS = 8192      # multigrid.hip: levels of at most this many vertices run in the single-workgroup kernel


@pytest.fixture(scope="module")
def levels():
    return np.load(mg_cases.LEVELS_GOLDEN)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
class Handle(object):
    def __init__(self, hip, dims):
        self.hip, self.dims = hip, dims
        self.h = ctypes.c_void_p()
        hip.lib.call("mf_mg_create", dims[0], dims[1], dims[2], ctypes.byref(self.h))

    def destroy(self):
        if self.h is not None:
            h, self.h = self.h, None
            self.hip.lib.call("mf_mg_destroy", h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def info(self):
        out = (ctypes.c_int64 * 72)()
        self.hip.lib.call("mf_mg_info", self.h, out, 72)
        nl = int(out[0])
        return dict(levels=nl, setups=int(out[1]), coarse_cg=int(out[2]), tail_first=int(out[5]),
                    sizes=[tuple(int(out[8 + 4 * l + c]) for c in range(3)) for l in range(nl)], active=[int(out[11 + 4 * l]) for l in range(nl)])

    def read(self, level, what, n):
        """one array of one level into a buffer pre-filled with NaN (types: 0xff)"""
        out = np.full(n, 0xff, np.uint8) if what == 0 else np.full((4 if level == 0 else 14, n) if what == 1 else n, np.nan, np.float32)
        self.hip.lib.call("mf_mg_read_level", self.h, level, what, out.ctypes.data_as(ctypes.c_void_p), out.nbytes)
        return out

    def set_a(self, A):
        dA = [self.hip.dev(a) for a in A]
        self.hip.call("mf_mg_set_a", self.h, dA[0], dA[1], dA[2], dA[3], None)
        self.hip.sync()
        for a, d in zip(A, dA):
            assert self.hip.host(d).tobytes() == np.ascontiguousarray(a).tobytes(), "mf_mg_set_a modified the caller's matrix"

    def vcycle(self, rhs):
        dst = self.hip.dev(np.full(rhs.shape, np.nan, np.float32))
        self.hip.call("mf_mg_vcycle", self.h, dst, self.hip.dev(rhs), None)
        self.hip.sync()
        return self.hip.host(dst)

    def state(self, cycled=True):
        """everything readable: info, and per level types, operator (rows of inactive vertices zeroed), b, x"""
        info = self.info()
        st = dict(info=info, t=[], A=[], b=[], x=[])
        for l, s in enumerate(info["sizes"]):
            n = s[0] * s[1] * s[2]
            t = self.read(l, 0, n)
            a = self.read(l, 1, n)
            a[:, t == 0] = 0
            st["t"].append(t); st["A"].append(a)
            if cycled:
                st["b"].append(self.read(l, 3, n)); st["x"].append(self.read(l, 2, n))
        return st


def _bits_differ(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "%s %s against %s %s" % (got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() == want.tobytes():
        return None
    view = np.uint8 if got.dtype == np.uint8 else np.int32
    bad = np.nonzero(got.reshape(-1).view(view) != want.reshape(-1).view(view))[0]
    i = int(bad[0])
    return "%d of %d values differ; first at %d: %r, expected %r" % (len(bad), got.size, i, got.reshape(-1)[i], want.reshape(-1)[i])


def sweep_order(nl):
    """(array, level) in the order in which a V-cycle produces them: the set-up, then the down sweep, then the up sweep"""
    return [(w, l) for l in range(nl) for w in ("t", "A")] + [("b", l) for l in range(nl)] + [("x", l) for l in range(nl - 1, -1, -1)]


NAMES = dict(t="vertex types", A="operator", b="b", x="x")


def assert_state_equals_model(st, H, cyc, what, active_only=False):
    """the first level and array that differs, in the order of the down sweep and then the up sweep"""
    assert st["info"]["levels"] == H.nl and st["info"]["sizes"] == H.sizes, (what, st["info"], H.sizes)
    assert st["info"]["active"] == H.active, (what, st["info"]["active"], H.active)
    for w, l in sweep_order(H.nl):
        if w in ("b", "x") and cyc is None:
            continue
        if w == "t":
            want = H.t[l]
        elif w == "A":
            want = H.A[l].copy()
            want[:, H.t[l] == 0] = 0
        else:
            want = cyc[w][l]
        got = st[w][l]
        if active_only and w in ("b", "x"):
            got, want = got[H.t[l] != 0], want[H.t[l] != 0]
        bad = _bits_differ(got, want)
        assert bad is None, "%s: %s of level %d differs from the model: %s" % (what, NAMES[w], l, bad)


def assert_state_equals_fixture(st, g, tag):
    nl = int(g[tag + "__levels"])
    assert st["info"]["levels"] == nl
    assert st["info"]["sizes"] == [tuple(int(v) for v in g[tag + "__size%d" % l]) for l in range(nl)]
    for w, l in sweep_order(nl):
        bad = mg_cases.recorded_mismatch(g, "%s__%s%d" % (tag, dict(t="type", A="A", b="b", x="x")[w], l), st[w][l])
        assert bad is None, "%s of level %d differs from the reference's: %s" % (NAMES[w], l, bad)


def expected_tail_first(sizes, tail_verts=TAIL_VERTS):
    first = len(sizes) - 1
    while first > 0 and sizes[first - 1][0] * sizes[first - 1][1] * sizes[first - 1][2] <= tail_verts:
        first -= 1
    return first


# ---- 1. levels, every edge case ----------------------------------------------------------------------------------------------------
_model_cache = {}


def model_of(g, tag):
    """dims, A, rhs, the model's hierarchy and its V-cycle for a recorded stage system; computed once per module run"""
    if tag not in _model_cache:
        dims, A, rhs = mg_cases.edge_stage_system(tag)
        H = mg_cases.model_hierarchy(g, tag, dims, A)
        _model_cache[tag] = (dims, A, rhs, H, M.vcycle(H, rhs))
    return _model_cache[tag]


@pytest.mark.parametrize("tag", mg_cases.edge_stage_tags())
def test_levels_equal_reference_and_model(hip, levels, tag):
    """after mf_mg_set_a: levels, sizes, active counts, tail_first, the types and the operator of every level; after one
    mf_mg_vcycle on the seeded rhs: b and x of every level, the result grid, the coarsest CG's iteration count -- against the
    recording and against the model.  A second V-cycle on the same handle repeats the first (x of the coarse levels is reset)."""
    dims, A, rhs, H, cyc = model_of(levels, tag)
    assert H.sizes == mg_cases.EDGE_LEVELS.get(dims, H.sizes)
    with Handle(hip, dims) as h:
        assert hip.lib.cdll.mf_mg_is_a_set(h.h) == 0
        h.set_a(A)
        assert hip.lib.cdll.mf_mg_is_a_set(h.h) == 1
        st = h.state(cycled=False)
        assert st["info"]["setups"] == 1
        assert st["info"]["tail_first"] == expected_tail_first(H.sizes)
        assert_state_equals_model(st, H, None, tag + " after set_a")
        result = h.vcycle(rhs)
        st = h.state()
        assert_state_equals_fixture(st, levels, tag)
        assert_state_equals_model(st, H, cyc, tag)
        bad = _bits_differ(result, cyc["result"])
        assert bad is None, "the result grid differs from x of level 0: " + bad
        assert st["info"]["coarse_cg"] == cyc["cg_iters"]
        again = h.vcycle(rhs)
        assert _bits_differ(again, result) is None, "a second V-cycle on the same handle differs from the first"
        assert h.info()["coarse_cg"] == cyc["cg_iters"] and h.info()["setups"] == 1


# ---- 2. the grid-wide form of every pass equals the tail form ----------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(33, 16, 16), (32, 16, 16), (21, 20, 19), (10, 10, 10)], ids=lambda d: "%dx%dx%d" % d)
def test_grid_wide_form_equals_tail_form(hip, levels, monkeypatch, dims):
    """MF_MG_TAIL_VERTS = 0 (the tail is the coarsest CG alone), unset (8192) and 1000000000 (every level in the tail): identical
    types, operators, b, x and result, each equal to the model; tail_first is what the setting implies"""
    tag = mg_cases.case_name("obs", dims) + "__lap"
    _, A, rhs, H, cyc = model_of(levels, tag)
    runs = []
    for setting, verts in (("0", 0), (None, TAIL_VERTS), ("1000000000", 10 ** 9)):
        if setting is None:
            monkeypatch.delenv("MF_MG_TAIL_VERTS", raising=False)
        else:
            monkeypatch.setenv("MF_MG_TAIL_VERTS", setting)      # read at every mf_mg_create
        with Handle(hip, dims) as h:
            h.set_a(A)
            result = h.vcycle(rhs)
            st = h.state()
        what = "%s with MF_MG_TAIL_VERTS=%s" % (tag, setting)
        assert st["info"]["tail_first"] == expected_tail_first(H.sizes, verts), what
        assert_state_equals_model(st, H, cyc, what)
        assert _bits_differ(result, cyc["result"]) is None, what
        assert st["info"]["coarse_cg"] == cyc["cg_iters"], what
        runs.append(st["info"]["tail_first"])
    assert runs[0] == H.nl - 1 and runs[2] == 0
    if dims == (33, 16, 16):
        assert runs == [2, 1, 0]      # level 0 (8448 vertices) is grid-wide by default
    if dims == (32, 16, 16):
        assert runs == [2, 0, 0]      # level 0 has exactly 8192 vertices: in the tail


# ---- 3. random systems beyond the fixture ------------------------------------------------------------------------------------------
def random_system(dims, seed, border_entries, block=False):
    """flags of util.make_flags with another seed and obstacles, their integer Laplace matrix, a rhs with values up to 1e3 and some
    exact zeros.  border_entries: the off-diagonal planes also get -1 in their LAST layer (Ai at x = sx - 1, ...), the entries
    that would couple to a vertex outside the grid: GridMg reads them when it classifies a row (analyzeStencil) and in no pass.
    block: a large obstacle block in the fluid, which leaves coarse vertices without any active fine vertex."""
    sx, sy, sz = dims
    flags = util.make_flags(sx, sy, sz, seed=seed, obstacles=True, empty_top=True)
    if block:
        flags[3:sz - 3, 2:(2 * sy) // 3 - 1, 3:sx - 3] = util.OBS
    A = [a.copy() for a in cases.run_laplace_impl(util.Impl("oracle"), dims, flags, None)]
    if border_entries:
        # rows in the outermost layers, so that the entries below belong to active vertices
        for sl in ((slice(None), slice(None), sx - 1), (slice(None), sy - 1, slice(None)), (sz - 1, slice(None), slice(None))):
            A[0][sl] = 6
        A[1][:, :, sx - 1] = -1
        A[2][:, sy - 1, :] = -1
        A[3][sz - 1] = -1
    rng = np.random.default_rng(seed + 100)
    rhs = (rng.uniform(-1e3, 1e3, (sz, sy, sx))).astype(np.float32)
    rhs[rng.random((sz, sy, sx)) < 0.2] = 0
    return A, rhs


RANDOM_CASES = [((10, 10, 10), 3, True), ((6, 5, 5), 4, True), ((33, 16, 16), 5, False), ((21, 20, 19), 6, True), ((64, 6, 5), 8, False)]


@pytest.mark.parametrize("dims,seed,border", RANDOM_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_random_systems_equal_model(hip, dims, seed, border):
    A, rhs = random_system(dims, seed, border)
    H = M.setup(dims, A)
    cyc = M.vcycle(H, rhs)
    assert cyc["cg_iters"] > 0 and np.isfinite(cyc["result"]).all()
    if border:
        assert H.t[0].reshape(dims[2], dims[1], dims[0])[:, :, dims[0] - 1].all() and (H.A[0][1].reshape(dims[2], dims[1], dims[0])[:, :, dims[0] - 1] == -1).all()
    with Handle(hip, dims) as h:
        h.set_a(A)
        result = h.vcycle(rhs)
        st = h.state()
    what = "random system %dx%dx%d seed %d" % (dims + (seed,))
    assert_state_equals_model(st, H, cyc, what)
    assert _bits_differ(result, cyc["result"]) is None, what
    assert st["info"]["coarse_cg"] == cyc["cg_iters"], what


# ---- 4. stale state ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(21, 20, 19), (33, 16, 16)], ids=lambda d: "%dx%dx%d" % d)
def test_second_set_a_equals_fresh_handle(hip, dims):
    """set_a(A), vcycle, set_a(B) with other flags on the same shape, vcycle: types, operators on active rows, b and x on active
    vertices and the result equal those of a fresh handle that was given only B (vertices that B leaves inactive keep what A left
    in their rows and vectors; nobody reads it)"""
    A, rhs_a = random_system(dims, 11, False)
    B, rhs_b = random_system(dims, 12, False, block=True)
    assert any((a != b).any() for a, b in zip(A, B))
    with Handle(hip, dims) as fresh, Handle(hip, dims) as used:
        fresh.set_a(B)
        want_result = fresh.vcycle(rhs_b)
        want = fresh.state()
        used.set_a(A)
        used.vcycle(rhs_a)
        was_active = [t != 0 for t in used.state()["t"]]
        used.set_a(B)
        got_result = used.vcycle(rhs_b)
        got = used.state()
    assert got["info"]["setups"] == 2 and want["info"]["setups"] == 1
    assert got["info"]["active"] == want["info"]["active"] and got["info"]["coarse_cg"] == want["info"]["coarse_cg"]
    # the case means something only if B switches vertices off that A had on, on level 0 and on a coarse level
    assert all(((t == 0) & was).any() for t, was in list(zip(want["t"], was_active))[:2]), "B leaves no vertex inactive that A had active"
    for w, l in sweep_order(want["info"]["levels"]):
        g_, w_ = got[w][l], want[w][l]
        if w in ("b", "x"):
            act = want["t"][l] != 0
            g_, w_ = g_[act], w_[act]
        bad = _bits_differ(g_, w_)      # operators: state() zeroed the rows of inactive vertices
        assert bad is None, "%s of level %d after the second set_a differs from a fresh handle's: %s" % (NAMES[w], l, bad)
    assert _bits_differ(got_result, want_result) is None
    H = M.setup(dims, B)
    assert_state_equals_model(got, H, M.vcycle(H, rhs_b), "second set_a", active_only=True)


# ---- 5. degenerate systems ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(10, 10, 10), (21, 20, 19)], ids=lambda d: "%dx%dx%d" % d)
def test_all_zero_matrix(hip, dims):
    sx, sy, sz = dims
    A = [np.zeros((sz, sy, sx), np.float32) for _ in range(4)]
    rhs = util.rand_real((sz, sy, sx), 5)
    with Handle(hip, dims) as h:
        h.set_a(A)
        result = h.vcycle(rhs)
        st = h.state()
    assert st["info"]["active"] == [0] * len(M.level_sizes(dims)) and st["info"]["coarse_cg"] == 0
    assert all((t == 0).all() for t in st["t"])
    assert _bits_differ(result, np.zeros_like(rhs)) is None, "V-cycle of the all-zero matrix"
    assert all(_bits_differ(x, np.zeros_like(x)) is None for x in st["x"])


@pytest.mark.parametrize("dims", [(10, 10, 10), (21, 20, 19)], ids=lambda d: "%dx%dx%d" % d)
def test_zero_rhs(hip, levels, dims):
    tag = mg_cases.case_name("liq", dims) + "__lap"
    _, A, rhs, H, _ = model_of(levels, tag)
    with Handle(hip, dims) as h:
        h.set_a(A)
        h.vcycle(rhs)      # leaves non-zero vectors on every level
        assert h.info()["coarse_cg"] > 0
        result = h.vcycle(np.zeros_like(rhs))
        st = h.state()
    assert st["info"]["coarse_cg"] == 0, "the coarsest CG runs on a zero residual"
    assert (result == 0).all() and not np.isnan(result).any()
    cyc = M.vcycle(H, np.zeros_like(rhs))
    assert cyc["cg_iters"] == 0
    assert_state_equals_model(st, H, cyc, "zero rhs", active_only=True)


# ---- 6. solves on the edge shapes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dims", mg_cases.EDGE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_edge_solve_equals_reference(hip_backend, levels, kind, dims):
    """solvePressure(preconditioner=PcMGDynamic) on the edge shapes: retRhs, pressure and velocity bit-exact against the compiled
    reference and the recorded digests; the iteration count is the recorded one and below 100"""
    flags, vel, phi, kw = mg_cases.inputs(kind, dims)
    name = mg_cases.case_name(kind, dims)
    want_iters = int(levels[name + "__iters"])
    assert want_iters < 100
    got = mg_cases.run_pkg(dims, flags, vel, phi, preconditioner=PcMGDynamic, **kw)
    print(name, "iterations", got["iterations"], "recorded", want_iters)
    want = mg_cases.run_ref(dims, flags, vel, phi, **kw)
    assert mg_cases.sha256(want["pressure"]) == bytes(levels[name + "__sha_p"]).hex(), "the compiled reference does not reproduce the recording"
    assert_bitexact(got["rhs"], want["rhs"], "retRhs")
    assert_bitexact(got["pressure"], want["pressure"], "pressure")
    assert_bitexact(got["vel"], want["vel"], "velocity")
    assert mg_cases.sha256(got["pressure"]) == bytes(levels[name + "__sha_p"]).hex()
    assert mg_cases.sha256(got["vel"]) == bytes(levels[name + "__sha_v"]).hex()
    assert got["iterations"] == want_iters
    if len(mg_cases.EDGE_LEVELS[dims]) == 1:
        ps = mg_cases.PkgSolver(dims)
        st = ps.solve(flags, vel, phi, preconditioner=PcMGStatic, **kw)      # Static keeps the hierarchy for a look
        assert ps.s._mg.info()["levels"] == 1 and ps.s._mg.info()["tail_first_level"] == 0
        assert_bitexact(st["pressure"], want["pressure"], "pressure of the Static solve")
        assert st["iterations"] == want_iters


def test_static_twice_on_one_level(hip_backend, levels):
    """PcMGStatic twice on 10 x 10 x 10: the second solve keeps the one-level hierarchy (setups == 1) and repeats the first"""
    dims = (10, 10, 10)
    flags, vel, phi, kw = mg_cases.inputs("obs", dims)
    ps = mg_cases.PkgSolver(dims)
    a = ps.solve(flags, vel, phi, preconditioner=PcMGStatic, **kw)
    mg = ps.s._mg
    assert mg.info()["levels"] == 1 and mg.info()["setups"] == 1
    b = ps.solve(flags, vel, phi, preconditioner=PcMGStatic, **kw)
    assert ps.s._mg is mg and mg.info()["setups"] == 1
    assert_bitexact(b["pressure"], a["pressure"], "second Static solve")
    assert mg_cases.sha256(a["pressure"]) == bytes(levels["obs_10x10x10__sha_p"]).hex()
    assert a["iterations"] == b["iterations"] == int(levels["obs_10x10x10__iters"])


# ---- 7. error returns --------------------------------------------------------------------------------------------------------------
def test_error_returns(hip, levels):
    """every refusal comes back non-zero with a message that names the entry point, and leaves the handle usable"""
    tag = "obs_11x10x10__lap"
    dims, A, rhs, H, cyc = model_of(levels, tag)
    sx, sy, sz = dims
    lib = hip.lib
    n = sx * sy * sz
    with Handle(hip, dims) as h:
        dst = hip.dev(np.full((sz, sy, sx), 7.0, np.float32))
        with pytest.raises(RuntimeError, match=r"mf_mg_vcycle: .*A has not been set"):
            hip.call("mf_mg_vcycle", h.h, dst, hip.dev(rhs), None)
        hip.sync()
        assert (hip.host(dst) == 7.0).all(), "a refused V-cycle wrote its result grid"
        # a solve with other dimensions than the handle's: all grids untouched
        odims = (sx, sy + 1, sz)
        grids = [hip.dev(np.full((odims[2], odims[1], odims[0]), 3.0, np.float32)) for _ in range(9)]
        oflags = hip.dev(util.make_flags(*odims, seed=1))
        out = (ctypes.c_float * 3)()
        with pytest.raises(RuntimeError, match=r"mf_mg_cg_solve: the hierarchy was created for 11 x 10 x 10, the system is 11 x 11 x 10"):
            hip.call("mf_mg_cg_solve", h.h, odims[0], odims[1], odims[2], oflags, *(grids + [ctypes.c_float(1e-3), 100, 0, out, None]))
        hip.sync()
        assert all((hip.host(g) == 3.0).all() for g in grids)
        assert lib.cdll.mf_mg_is_a_set(h.h) == 0
        buf = np.zeros(14 * n, np.float32)
        p = buf.ctypes.data_as(ctypes.c_void_p)
        for level, what, nbytes, msg in ((-1, 0, n, r"mf_mg_read_level: level -1 of 2"), (2, 0, n, r"mf_mg_read_level: level 2 of 2"),
                                         (0, 4, n, r"mf_mg_read_level: what = 4"), (0, -1, n, r"mf_mg_read_level: what = -1"),
                                         (0, 0, n + 1, r"mf_mg_read_level: %d bytes given, the array has %d" % (n + 1, n)),
                                         (0, 1, 14 * 4 * n, r"mf_mg_read_level: %d bytes given, the array has %d" % (56 * n, 16 * n)),
                                         (1, 2, 4 * n, r"mf_mg_read_level: %d bytes given, the array has %d" % (4 * n, 4 * 216))):
            with pytest.raises(RuntimeError, match=msg):
                lib.call("mf_mg_read_level", h.h, level, what, p, nbytes)
        assert (buf == 0).all()
        short = (ctypes.c_int64 * 72)()
        with pytest.raises(RuntimeError, match=r"mf_mg_info: out_host holds 15 entries, 16 needed"):
            lib.call("mf_mg_info", h.h, short, 15)
        assert not any(short)
        # the handle is still usable: set_a + vcycle equal the model
        h.set_a(A)
        result = h.vcycle(rhs)
        assert_state_equals_model(h.state(), H, cyc, tag + " after the refusals")
        assert _bits_differ(result, cyc["result"]) is None
        dead = ctypes.c_void_p(h.h.value)
        h.destroy()
    # a destroyed handle, and no handle at all
    for bad in (dead, ctypes.c_void_p()):
        assert lib.cdll.mf_mg_is_a_set(bad) == -1
        for name, args in (("mf_mg_destroy", ()), ("mf_mg_vcycle", (None, None, None)), ("mf_mg_set_a", (None, None, None, None, None)),
                           ("mf_mg_info", ((ctypes.c_int64 * 72)(), 72)), ("mf_mg_read_level", (0, 0, p, n))):
            with pytest.raises(RuntimeError, match=name + ": bad handle"):
                lib.call(name, bad, *args)
    with pytest.raises(RuntimeError, match=r"mf_mg_create: .*3-D only"):
        lib.call("mf_mg_create", 12, 12, 1, ctypes.byref(ctypes.c_void_p()))
