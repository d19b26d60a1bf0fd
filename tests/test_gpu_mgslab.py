"""-m gpu: the ranged level-0 entries of include/open/manta_hip_mgslab.h, driven as P pretend-ranks inside one process: P
separate handles of mf_mg_create with the same matrix, the plane exchanges and the all-gather of b of level 1 as plane copies
between them (mf_mgslab_get_planes / _put_planes), in the schedule of mantaflow_amd/slab.py (tests/mgslab_model.py states it on
the CPU).  Level 0's x, b and r of every pretend-rank start as NaN, so a pass that reads a plane the schedule did not bring
there shows.  Everything is compared bit for bit with one mf_mg_vcycle on a fresh handle: dst, and x and b of every level.

Shapes: 24 x 20 x 18 and 24 x 20 x 19 (8640 and 9120 vertices, just above the 8192-vertex hand-over: level 0 is grid-wide, the
levels below run in the tail; even and odd NZ), 12 x 10 x 9 with MF_MG_TAIL_VERTS=0 (a child process: the tail is the coarsest
CG alone), 12 x 10 x 9 as it comes (level 0 inside the tail: not cut, the replicated fallback) and 10^3 (one level)."""
import ctypes
import os
import subprocess
import sys

if __name__ == "__main__":      # the child process of the MF_MG_TAIL_VERTS case: the package is imported from the tree
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest

import mgslab_cases as C
from mgslab_model import coarse_planes

pytestmark = pytest.mark.gpu

X, B, R = 2, 3, 4


class Handle(object):
    def __init__(self, hip, dims):
        self.hip, self.dims = hip, dims
        self.h = ctypes.c_void_p()
        hip.lib.call("mf_mg_create", dims[0], dims[1], dims[2], ctypes.byref(self.h))
        out = (ctypes.c_int64 * 72)()
        hip.lib.call("mf_mg_info", self.h, out, 72)
        self.levels, self.tail_first = int(out[0]), int(out[5])
        self.sizes = [tuple(int(out[8 + 4 * l + c]) for c in range(3)) for l in range(self.levels)]

    def destroy(self):
        if self.h is not None:
            h, self.h = self.h, None
            self.hip.lib.call("mf_mg_destroy", h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def n(self, level):
        s = self.sizes[level]
        return s[0] * s[1] * s[2]

    def set_a(self, A):
        dA = [self.hip.dev(a) for a in A]
        self.hip.call("mf_mg_set_a", self.h, dA[0], dA[1], dA[2], dA[3], None)
        self.hip.sync()

    def call(self, name, *args):
        self.hip.call(name, self.h, *args)

    def get(self, level, what, z0, z1):
        """planes [z0, z1) of a vector of a level -> numpy"""
        s = self.sizes[level]
        out = self.hip.dev(np.full((z1 - z0) * s[0] * s[1], np.nan, np.float32))
        self.call("mf_mgslab_get_planes", level, what, z0, z1, out, None)
        self.hip.sync()
        return self.hip.host(out)

    def put(self, level, what, z0, a):
        s = self.sizes[level]
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        self.call("mf_mgslab_put_planes", level, what, z0, z0 + a.size // (s[0] * s[1]), self.hip.dev(a), None)
        self.hip.sync()

    def whole(self, level, what):
        return self.get(level, what, 0, self.sizes[level][2])

    def vcycle(self, rhs):
        dst = self.hip.dev(np.full(rhs.shape, np.nan, np.float32))
        self.call("mf_mg_vcycle", dst, self.hip.dev(rhs), None)
        self.hip.sync()
        return self.hip.host(dst)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, what
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    assert bad.size == 0, "%s: %d of %d values differ; first at %d: %r, expected %r" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def cut_vcycle(hs, rhs, ranges):
    """the schedule of slab.SlabMG.vcycle on the pretend-ranks hs -> dst per rank (its owned planes)"""
    sx, sy, NZ = hs[0].dims
    XY = sx * sy
    P = len(hs)
    hip = hs[0].hip

    def exchange(what):
        send = [(h.get(0, what, z0, z0 + 1), h.get(0, what, z1 - 1, z1)) for h, (z0, z1) in zip(hs, ranges)]
        for q, (h, (z0, z1)) in enumerate(zip(hs, ranges)):
            if q > 0:
                h.put(0, what, z0 - 1, send[q - 1][1])
            if q < P - 1:
                h.put(0, what, z1, send[q + 1][0])

    def each(name, *args, planes=None):
        for h, (z0, z1) in zip(hs, ranges):
            a, b = (z0, z1) if planes is None else planes(z0, z1)
            h.call(name, *(args + (a, b, None)))

    nan = np.full(NZ * XY, np.nan, np.float32)
    for h, (z0, z1) in zip(hs, ranges):
        for what in (X, B, R):
            h.put(0, what, 0, nan)
        h.call("mf_mgslab_set_rhs", z0, z1, hip.dev(rhs[z0 * XY:z1 * XY]), None)
    each("mf_mgslab_smooth", 0)
    exchange(X)
    each("mf_mgslab_smooth", 1)
    exchange(X)
    each("mf_mgslab_residual")
    exchange(R)
    each("mf_mgslab_restrict", planes=lambda z0, z1: coarse_planes(z0, z1, NZ))
    # the all-gather: every coarse plane from its owner into every other rank
    cr = [coarse_planes(z0, z1, NZ) for z0, z1 in ranges]
    rows = [h.get(1, B, k0, k1) if k1 > k0 else None for h, (k0, k1) in zip(hs, cr)]
    for q, h in enumerate(hs):
        for p in range(P):
            if p != q and rows[p] is not None:
                h.put(1, B, cr[p][0], rows[p])
    for h in hs:
        h.call("mf_mgslab_coarse", None)
    each("mf_mgslab_interp_add", planes=lambda z0, z1: (max(z0 - 1, 0), min(z1 + 1, NZ)))
    each("mf_mgslab_smooth", 1)
    exchange(X)
    each("mf_mgslab_smooth", 0)
    return [h.get(0, X, z0, z1) for h, (z0, z1) in zip(hs, ranges)]


def check_cut_form(hip, dims, kind, cuts):
    """P pretend-ranks against one mf_mg_vcycle on a fresh handle: dst, and x and b of every level"""
    A, rhs = C.system(kind, dims)
    XY = dims[0] * dims[1]
    ranges = C.ranges_of(dims[2], cuts)
    with Handle(hip, dims) as ref:
        ref.set_a(A)
        assert ref.levels >= 2 and ref.tail_first >= 1, "this case must take the cut form"
        want = ref.vcycle(rhs)
        want_x = [ref.whole(l, X) for l in range(ref.levels)]
        want_b = [ref.whole(l, B) for l in range(ref.levels)]
        _same(want, want_x[0], "the undivided result is x of level 0")
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        hs = [Handle(hip, dims) for _ in ranges]
        try:
            for h in hs:
                h.set_a(A)
            dst = cut_vcycle(hs, rhs, ranges)
            for q, (h, (z0, z1)) in enumerate(zip(hs, ranges)):
                tag = "%s %s cuts %r rank %d" % ("x".join(str(d) for d in dims), kind, cuts, q)
                _same(dst[q], want[z0 * XY:z1 * XY], tag + ": dst on the owned planes")
                _same(h.get(0, B, z0, z1), want_b[0][z0 * XY:z1 * XY], tag + ": b of level 0 on the owned planes")
                for l in range(1, ref.levels):
                    _same(h.whole(l, B), want_b[l], tag + ": b of level %d" % l)
                    _same(h.whole(l, X), want_x[l], tag + ": x of level %d" % l)
        finally:
            for h in hs:
                h.destroy()


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("dims,cuts", [((24, 20, 18), (9,)), ((24, 20, 18), (6, 12)), ((24, 20, 19), (9,)), ((24, 20, 19), (6, 12))],
                         ids=lambda v: "x".join(str(i) for i in v))
def test_cut_form_equals_undivided_vcycle(hip, dims, cuts, kind):
    assert "MF_MG_TAIL_VERTS" not in os.environ
    check_cut_form(hip, dims, kind, cuts)


@pytest.mark.parametrize("kind", C.KINDS)
def test_cut_form_with_the_tail_reduced_to_the_coarsest_cg(kind):
    """12 x 10 x 9 with MF_MG_TAIL_VERTS=0 (read at mf_mg_create, so a child process): two levels, level 0 grid-wide, the tail is the
    coarsest CG alone; worlds 2 and 3, a cut at an odd plane and a one-plane slab at an odd plane"""
    env = dict(os.environ, MF_MG_TAIL_VERTS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), kind], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("dims", [(12, 10, 9), (10, 10, 10)], ids=lambda d: "x".join(str(i) for i in d))
def test_level_0_inside_the_tail_is_not_cut(hip, dims, kind):
    """12 x 10 x 9 as it comes (two levels, both in the single-workgroup tail) and 10^3 (one level): mf_mgslab_coarse refuses by name,
    and the replicated fallback -- mf_mg_vcycle on the whole rhs on every rank, the owned planes taken -- is the undivided result"""
    assert "MF_MG_TAIL_VERTS" not in os.environ
    A, rhs = C.system(kind, dims)
    XY = dims[0] * dims[1]
    with Handle(hip, dims) as ref:
        ref.set_a(A)
        assert ref.tail_first == 0 and ref.levels == (2 if dims == (12, 10, 9) else 1)
        want = ref.vcycle(rhs)
        with pytest.raises(RuntimeError, match=r"^mf_mgslab_coarse: level 0 of this hierarchy runs inside the single-workgroup tail"):
            ref.call("mf_mgslab_coarse", None)
        if ref.levels == 1:
            with pytest.raises(RuntimeError, match=r"^mf_mgslab_restrict: the hierarchy has one level"):
                ref.call("mf_mgslab_restrict", 0, 1, None)
            with pytest.raises(RuntimeError, match=r"^mf_mgslab_interp_add: the hierarchy has one level"):
                ref.call("mf_mgslab_interp_add", 0, 1, None)
        _same(ref.whole(0, X), want, "nothing was touched by the refusals")
        for cuts in ((5,), (3, 4)):
            for z0, z1 in C.ranges_of(dims[2], cuts):
                with Handle(hip, dims) as h:
                    h.set_a(A)
                    _same(h.vcycle(rhs)[z0 * XY:z1 * XY], want[z0 * XY:z1 * XY], "replicated fallback, planes [%d, %d)" % (z0, z1))


def test_ranged_passes_leave_other_planes_alone(hip):
    """every ranged entry on planes [z0, z1) of a handle whose vectors hold a sentinel pattern: every plane outside what the entry
    is documented to write keeps its bits, and the planes inside change"""
    dims = (24, 20, 19)
    A, rhs = C.system("trivial_gf", dims)
    XY = dims[0] * dims[1]
    rng = np.random.RandomState(7)
    with Handle(hip, dims) as h:
        h.set_a(A)
        n0, n1, cXY = h.n(0), h.n(1), h.sizes[1][0] * h.sizes[1][1]
        sent0 = {w: rng.uniform(1.0, 2.0, n0).astype(np.float32) for w in (X, B, R)}
        sent1 = {w: rng.uniform(1.0, 2.0, n1).astype(np.float32) for w in (X, B)}

        def reset():
            for w, a in sent0.items():
                h.put(0, w, 0, a)
            for w, a in sent1.items():
                h.put(1, w, 0, a)

        def check(name, written):
            """written: {(level, what): (a, b)} -- the planes the entry may write"""
            for (level, w), sent in [((0, k), v) for k, v in sent0.items()] + [((1, k), v) for k, v in sent1.items()]:
                got = h.whole(level, w)
                pl = XY if level == 0 else cXY
                a, b = written.get((level, w), (0, 0))
                _same(got[:a * pl], sent[:a * pl], "%s: level %d vector %d below plane %d" % (name, level, w, a))
                _same(got[b * pl:], sent[b * pl:], "%s: level %d vector %d from plane %d" % (name, level, w, b))
                if b > a:
                    assert (got[a * pl:b * pl].view(np.int32) != sent[a * pl:b * pl].view(np.int32)).any(), "%s wrote nothing" % name

        for z0, z1 in ((6, 12), (0, 5), (13, 19), (7, 8)):
            reset()
            h.call("mf_mgslab_set_rhs", z0, z1, hip.dev(rhs[z0 * XY:z1 * XY]), None)
            check("set_rhs", {(0, B): (z0, z1), (0, X): (max(z0 - 1, 0), min(z1 + 1, dims[2]))})
            for colour in (0, 1):
                reset()
                h.call("mf_mgslab_smooth", colour, z0, z1, None)
                check("smooth %d" % colour, {(0, X): (z0, z1)})
            reset()
            h.call("mf_mgslab_residual", z0, z1, None)
            check("residual", {(0, R): (z0, z1)})
            reset()
            h.call("mf_mgslab_interp_add", z0, z1, None)
            check("interp_add", {(0, X): (z0, z1)})
            k0, k1 = coarse_planes(z0, z1, dims[2])
            reset()
            h.call("mf_mgslab_restrict", k0, k1, None)
            check("restrict", {(1, B): (k0, k1), (1, X): (k0, k1)})      # knSet(x_1, 0) rides in the restriction
            # an empty range is a no-op
            reset()
            for name, args in (("mf_mgslab_smooth", (0, z0, z0)), ("mf_mgslab_residual", (z0, z0)), ("mf_mgslab_interp_add", (z1, z1)),
                               ("mf_mgslab_restrict", (k0, k0)), ("mf_mgslab_set_rhs", (z0, z0, None))):
                h.call(name, *(args + (None,)))
            check("empty ranges", {})


def test_entries_refuse_by_name(hip):
    dims = (24, 20, 19)
    A, rhs = C.system("lap", dims)
    XY = dims[0] * dims[1]
    buf = hip.dev(np.zeros(dims[2] * XY, np.float32))
    calls = [("mf_mgslab_set_rhs", (2, 4, buf, None)), ("mf_mgslab_smooth", (0, 2, 4, None)), ("mf_mgslab_residual", (2, 4, None)),
             ("mf_mgslab_restrict", (1, 2, None)), ("mf_mgslab_coarse", (None,)), ("mf_mgslab_interp_add", (2, 4, None)),
             ("mf_mgslab_get_planes", (0, X, 2, 4, buf, None)), ("mf_mgslab_put_planes", (0, X, 2, 4, buf, None)),
             ("mf_mgslab_set_accuracy", (1e-3,))]

    def refused(handle, name, args, pattern):
        with pytest.raises(RuntimeError, match=pattern):
            hip.call(name, handle, *args)

    # an unset matrix
    with Handle(hip, dims) as h:
        for name, args in calls:
            refused(h.h, name, args, r"^%s: GridMg::setRhs Error: A has not been set\.$" % name)
        h.set_a(A)
        want = h.vcycle(rhs)
        # plane ranges outside the level, reversed ranges, levels and vectors that do not exist, a colour level 0 does not have
        for name, args in (("mf_mgslab_set_rhs", (-1, 4, buf, None)), ("mf_mgslab_set_rhs", (2, 20, buf, None)), ("mf_mgslab_smooth", (0, 5, 4, None)),
                           ("mf_mgslab_residual", (0, 20, None)), ("mf_mgslab_restrict", (0, h.sizes[1][2] + 1, None)),
                           ("mf_mgslab_interp_add", (-2, 3, None)), ("mf_mgslab_get_planes", (1, B, 0, h.sizes[1][2] + 1, buf, None)),
                           ("mf_mgslab_put_planes", (0, R, 19, 20, buf, None))):
            refused(h.h, name, args, r"^%s: plane range \[-?\d+, -?\d+\) outside the \d+ planes of level \d$" % name)
        refused(h.h, "mf_mgslab_get_planes", (h.levels, X, 0, 1, buf, None), r"^mf_mgslab_get_planes: level %d of %d$" % (h.levels, h.levels))
        refused(h.h, "mf_mgslab_put_planes", (-1, X, 0, 1, buf, None), r"^mf_mgslab_put_planes: level -1 of")
        refused(h.h, "mf_mgslab_get_planes", (0, 1, 0, 1, buf, None), r"^mf_mgslab_get_planes: what = 1")
        refused(h.h, "mf_mgslab_smooth", (2, 2, 4, None), r"^mf_mgslab_smooth: colour 2")
        _same(h.whole(0, X), want, "x of level 0 after the refusals")
        dead = ctypes.c_void_p(h.h.value)
    # a destroyed handle, a pointer nobody handed out, a null pointer, a 2-D handle
    two_d = ctypes.c_void_p()
    hip.lib.call("mf_mg2d_create", 24, 20, ctypes.byref(two_d))
    try:
        stray = (ctypes.c_char * 4096)()
        for handle in (dead, ctypes.c_void_p(ctypes.addressof(stray)), None, two_d):
            for name, args in calls:
                refused(handle, name, args, r"^%s: bad handle \(not a live 3-D hierarchy of mf_mg_create\)$" % name)
    finally:
        hip.lib.call("mf_mg2d_destroy", two_d)


if __name__ == "__main__":
    # the child of test_cut_form_with_the_tail_reduced_to_the_coarsest_cg: MF_MG_TAIL_VERTS=0 is in the environment
    import util
    assert os.environ.get("MF_MG_TAIL_VERTS") == "0"
    impl = util.Impl("hip")
    for cuts in ((5,), (4,), (3, 4), (2, 6)):
        check_cut_form(impl, (12, 10, 9), sys.argv[1], cuts)
    print("ok")
