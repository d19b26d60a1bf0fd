"""mf_cg_solve on every route it can take, iterate by iterate, with incoming values that break the premise of its liquid-scene
shortcut, and mf_apply_matrix at the grid's ends -- on the HIP library against the oracle (and the compiled reference where it
travelled).  tests/test_oracle_pcg_routes.py pins the oracle to the reference on the same inputs.

The bars of the solves are those of test_gpu_parity.test_cg_solve: the same iteration count, dst within 1e-5 relative, resNorm and
sigma within 1e-4.  ApplyMatrix and the MIC apply are bit-exact."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cases
import util
from util import assert_bitexact, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _close(a, b, what, tol=TOL):
    e = rel_err(a, b)
    assert e <= tol, "%s: relative error %g > %g" % (what, e, tol)


def _solve(impl, dims, flags, A, rhs, pc, acc, iters, l2=0, work=None):
    """(dst, (iterations, resNorm, sigma)), or None when the solver reported divergence (conjugategrad.cpp:288-295)"""
    try:
        return cases.run_cg_impl(impl, dims, flags, A, rhs, pc, acc, iters, l2, work=work)
    except RuntimeError as e:
        if "diverged" not in str(e):
            raise
        return None


def _solve_ref(dims, flags, A, rhs, pc, acc, iters, l2=0, work=None):
    try:
        return cases.run_cg_ref(dims, flags, A, rhs, pc, acc, iters, l2, work=work)
    except RuntimeError as e:
        if "diverged" not in str(e):
            raise
        return None


def _agree(got, want, what):
    if got is None or want is None:
        assert got is None and want is None, "%s: only one side diverged (%s / %s)" % (what, got and got[1], want and want[1])
        return
    assert got[1][0] == want[1][0], "%s: iterations %s vs %s" % (what, got[1], want[1])
    _close(got[0], want[0], what + ": dst")
    _close(got[1][1:], want[1][1:], what + ": resNorm/sigma", 1e-4)


def _check_solve(hip, oracle, dims, flags, A, rhs, pc, acc, iters, l2=0, work=None, what=""):
    got = _solve(hip, dims, flags, A, rhs, pc, acc, iters, l2, work)
    sc = _shortcut(hip)
    want = _solve(oracle, dims, flags, A, rhs, pc, acc, iters, l2, work)
    _agree(got, want, what + " (oracle)")
    if util.have_ref():
        _agree(got, _solve_ref(dims, flags, A, rhs, pc, acc, iters, l2, work), what + " (reference)")
    return got, want, sc


def _shortcut(hip):
    sc = (ctypes.c_int32 * 3)()
    assert hip.lib.cdll.mf_cg_last_shortcut(sc) == 0
    return list(sc)


# ---- the route table (cases.PCG_ROUTES names the route of each shape) ----
ROUTES = [pytest.param(d, pc, id="%dx%dx%d-pc%d" % (d + (pc,))) for d, _ in cases.PCG_ROUTES for pc in ((2, 0) if d[2] > 1 else (0,))]


@pytest.mark.parametrize("dims,pc", ROUTES)
@pytest.mark.parametrize("acc,iters", [(1e-9, 4), (1e-3, 400)], ids=["stopping", "converging"])
@pytest.mark.parametrize("l2", [0, 1])
def test_cg_route(hip, oracle, dims, pc, acc, iters, l2):
    flags, A, _ = cases.system_inputs(dims, 5)
    rhs = cases.cg_rhs(dims, flags, 5)
    got, want, _ = _check_solve(hip, oracle, dims, flags, A, rhs, pc, acc, iters, l2, what="%s pc %d" % (dims, pc))
    if acc > 1e-6:
        assert 0 < want[1][0] < iters, want[1]     # a converging case converges


# ---- iterate by iterate: one shape per route, maxIter = 1 ... 12 from the same inputs ----
ITERATE = [((13, 11, 9), 2), ((13, 11, 9), 0), ((12, 10, 7), 2), ((17, 9, 10), 2), ((63, 18, 10), 2), ((16, 67, 5), 2),
           ((24, 9, 70), 2), ((37, 29, 1), 0), ((64, 33, 1), 0)]


@pytest.mark.parametrize("dims,pc", [pytest.param(d, pc, id="%dx%dx%d-pc%d" % (d + (pc,))) for d, pc in ITERATE])
def test_cg_iterate_by_iterate(hip, oracle, dims, pc):
    """a wrong alpha, beta or preconditioner apply that later iterations would correct shows in the iterate after k steps"""
    flags, A, _ = cases.system_inputs(dims, 5)
    rhs = cases.cg_rhs(dims, flags, 5)
    for k in range(1, 13):
        got = cases.run_cg_impl(hip, dims, flags, A, rhs, pc, 1e-7, k)
        want = cases.run_cg_impl(oracle, dims, flags, A, rhs, pc, 1e-7, k)
        _agree(got, want, "%s pc %d after %d iterations" % (dims, pc, k))
        if want[1][0] < k:
            break
        assert got[1][0] == k


# ---- liquid scenes ----
def test_cg_liquid_many_bundles_per_workgroup(hip, oracle):
    """a liquid sweep with more 8 x 8 row bundles than the device has CUs: each workgroup of the sweep draws several bundles, and the
    dot shares of its empty bundles ride on the residual update (pcg_setup's be_map)"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    nb = math.isqrt(cu) + 1                                      # nb * nb bundles > cu
    dims = (32, 8 * nb, 8 * nb)
    box = (9, 20, 1, 4 * nb, 1, 8 * nb - 1)
    flags, A, rhs = cases.liquid_box_system(dims, box, 13)
    got, want, sc = _check_solve(hip, oracle, dims, flags, A, rhs, 2, 1e-3, 60, what="%s liquid" % (dims,))
    assert 3 < want[1][0] < 60, want[1]
    assert sc == [1, 8, 16], sc                                  # bundles skipped, sweeps trimmed to the chunks [8, 24)


def test_solve_pressure_fused_partial_bundles(hip, oracle):
    """mf_solve_pressure_fused (matrix-free set-up) against the three calls it stands for, on the HIP library and the oracle, at a shape
    whose last bundles of rows are partial in y and z"""
    dims = (32, 21, 19)
    sx, sy, sz = dims
    flags, vel, _ = cases.pressure_inputs(dims, 7, True)      # (an empty band on top: the solve converges)
    res = {}
    for name, impl in (("hip", hip), ("oracle", oracle)):
        f, v = impl.dev(flags), impl.dev(vel)
        g = [impl.dev(np.zeros((sz, sy, sx), np.float32)) for _ in range(6)]
        out = (ctypes.c_float * 3)()
        impl.call("mf_solve_pressure_fused", sx, sy, sz, f, v, g[0], g[1], g[2], g[3], g[4], g[5], 1e-3, 200, 0, out, None)
        impl.sync()
        res[name, "fused"] = (impl.host(g[0]), impl.host(g[1]), int(out[0]))
        p, rhs, r_, s_, t_, ap = [impl.dev(np.zeros((sz, sy, sx), np.float32)) for _ in range(6)]
        A = [impl.dev(np.zeros((sz, sy, sx), np.float32)) for _ in range(4)]
        impl.call("mf_make_rhs", sx, sy, sz, f, rhs, v, None, None, None, None, None, 0.0, 1e-4, None, None, None)
        impl.call("mf_make_laplace_matrix", sx, sy, sz, f, *A, None, None)
        out = (ctypes.c_float * 3)()
        impl.call("mf_cg_solve", sx, sy, sz, f, p, rhs, r_, s_, t_, *A, ap, 2, 1e-3, 200, 0, out, None)
        impl.sync()
        res[name, "calls"] = (impl.host(p), impl.host(rhs), int(out[0]))
    want = res["oracle", "calls"]
    assert 3 < want[2] < 200, want[2]
    for key in (("hip", "fused"), ("hip", "calls"), ("oracle", "fused")):
        got = res[key]
        assert got[2] == want[2], (key, got[2], want[2])
        assert_bitexact(got[1], want[1], "%s rhs" % (key,))
        _close(got[0], want[0], "%s pressure" % (key,))


# ---- the premise of the liquid-scene shortcut (include/manta_hip.h at mf_cg_solve) ----
PREMISE = ["clean", "rhs_empty_bundle", "rhs_minus_zero", "tmp_empty_bundle", "tmp_beside_fluid", "search_nonfluid", "rhs_outside_xrange"]
# variants in which something other than +0 sits where the shortcut needs +0: mf_cg_last_shortcut must report neither skipping nor trim
BROKEN = {"rhs_empty_bundle", "rhs_minus_zero", "tmp_empty_bundle", "rhs_outside_xrange"}
PREMISE_CASES = [pytest.param(d, box, v, id="%dx%dx%d-%s" % (d + (v,))) for d, box, _ in cases.LIQUID_SHORTCUT for v in PREMISE
                 if v != "rhs_outside_xrange" or box[1] + 9 < d[0]]


@pytest.mark.parametrize("dims,box,variant", PREMISE_CASES)
def test_cg_shortcut_premise(hip, oracle, dims, box, variant):
    """incoming rhs / tmp / search values outside the fluid: the reference carries them through the iteration (a rhs that is not zero
    there is solved without the shortcut); the HIP solve must give the same answer on every route, shortcut or not"""
    sx = dims[0]
    x0, x1 = box[0], box[1]
    flags, A, rhs = cases.liquid_box_system(dims, box, 9)
    edit, work = cases.liquid_variants(dims, box, flags)[variant]
    rhs = rhs.copy()
    for cell, v in (edit or {}).items():
        rhs[cell] = v
    _, want, sc = _check_solve(hip, oracle, dims, flags, A, rhs, 2, 1e-4, 30, 0, work, what="%s %s" % (dims, variant))
    if variant == "clean":
        assert want is not None and 3 < want[1][0] < 30, want and want[1]
        if sx % 8 == 0 or sx >= 16:
            # bundles skipped, sweeps trimmed to the chunks of 8 cells around [x0, x1] (plus the cell its last Ai bit couples)
            assert sc == [1, (x0 // 8) * 8, min(((x1 + 1 + 7) // 8) * 8, ((sx + 7) // 8) * 8) - (x0 // 8) * 8], sc
    if sx % 8 != 0 and sx < 16:
        assert sc[1:] == [0, 0], sc                              # never trimmed: the x-range needs sx % 8 == 0
    if variant in BROKEN:
        assert sc == [0, 0, 0], sc


@pytest.mark.parametrize("dims,box", [pytest.param(d, box, id="%dx%dx%d" % d) for d, box, _ in cases.LIQUID_SHORTCUT])
def test_mic_apply_keeps_dst_outside_the_fluid(hip, oracle, dims, box):
    """mf_mic_apply on the system mf_mic_init registered (empty bundles left out): dst keeps its previous content in every non-fluid
    cell, as the reference does, and the fluid cells have the oracle's bits"""
    sx, sy, sz = dims
    flags, A, _ = cases.liquid_box_system(dims, box, 9)
    var1 = util.rand_real((sz, sy, sx), 17)
    sentinel = np.float32(-7.25)
    outs = {}
    for name, impl in (("hip", hip), ("oracle", oracle)):
        f, dA = impl.dev(flags), [impl.dev(a) for a in A]
        ap = impl.dev(np.zeros((sz, sy, sx), np.float32))
        impl.call("mf_mic_init", sx, sy, sz, f, ap, *dA, None)
        dst = impl.dev(np.full((sz, sy, sx), sentinel, np.float32))
        impl.call("mf_mic_apply", sx, sy, sz, f, dst, impl.dev(var1), ap, dA[1], dA[2], dA[3], None)
        impl.sync()
        outs[name] = impl.host(dst)
    nonfluid = (flags & util.FLUID) == 0
    assert (outs["hip"][nonfluid].view(np.uint32) == sentinel.view(np.uint32)).all(), \
        "%d non-fluid cells changed" % (outs["hip"][nonfluid] != sentinel).sum()
    assert_bitexact(outs["hip"], outs["oracle"], "MIC apply")
    if util.have_ref():
        ap_r = np.zeros((sz, sy, sx), np.float32)
        util.refcall("ref_mic_init", sx, sy, sz, flags, ap_r, *A)
        dst_r = np.full((sz, sy, sx), sentinel, np.float32)
        util.refcall("ref_mic_apply", sx, sy, sz, flags, dst_r, var1, ap_r, *A)
        assert_bitexact(outs["hip"], dst_r, "MIC apply (reference)")


# ---- ApplyMatrix at the grid's ends, on every dispatch path of launch_apply_matrix ----
EDGE = [
    ("v5", (16, 12, 6), False, 0),
    ("v5-odd-sy", (16, 11, 7), False, 0),
    ("v5-longrows", (260, 7, 4), False, 0),                     # rows longer than a wave: +-X neighbours across lane 63 / 0
    ("v5-packed", (16, 12, 6), True, 0),
    ("v5-packed-odd-sy", (24, 9, 5), True, 0),
    ("v5-2d", (16, 12, 1), False, 0),
    ("v5-2d-odd-sy", (20, 11, 1), False, 0),
    ("scalar-sx13", (13, 10, 6), False, 0),
    ("scalar-2d-sx13", (13, 10, 1), False, 0),
    ("scalar-offset-views", (16, 12, 6), False, 1),             # every view one float into an allocation of n + 1 floats
]


def _apply_matrix(impl, dims, flags, A, src, packed, offset):
    sx, sy, sz = dims
    n = sx * sy * sz

    def view(a):
        t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
        buf = torch.zeros(n + offset, dtype=t.dtype, device=impl.device)
        buf[offset:].copy_(t)
        return buf[offset:]

    f, s_, dA = view(flags), view(src), [view(a) for a in A]
    dst = view(np.full((sz, sy, sx), 7.0, np.float32))
    if packed:
        impl.call("mf_pack_matrix", sx, sy, sz, f, *dA, None)
    impl.call("mf_apply_matrix", sx, sy, sz, f, dst, s_, *dA, None)
    impl.sync()
    out = impl.host(dst).reshape((sz, sy, sx)).copy()
    if packed:
        # drop the packed bytes: a matrix that is not all +0 / -1 replaces them (freed pointers must not stay registered)
        B = [a.clone() for a in dA]
        B[1].fill_(0.5)
        impl.call("mf_pack_matrix", sx, sy, sz, f, *B, None)
        impl.sync()
    return out


@pytest.mark.parametrize("name,dims,packed,offset", [pytest.param(*e, id=e[0]) for e in EDGE])
def test_apply_matrix_grid_ends(hip, oracle, name, dims, packed, offset):
    """caller-built couplings across row ends and plane ends, fluid on the domain border, large finite and -0.0 operands in the
    non-fluid cells: the flat indexing of conjugategrad.h:118-151, bit for bit"""
    flags, A, src = cases.apply_matrix_edge_inputs(dims, 3, packed)
    got = _apply_matrix(hip, dims, flags, A, src, packed, offset)
    want = _apply_matrix(oracle, dims, flags, A, src, packed, 0)
    assert_bitexact(got, want, "%s ApplyMatrix" % name)
    if util.have_ref():
        assert_bitexact(got, cases.run_apply_matrix_ref(dims, flags, A, src), "%s ApplyMatrix (reference)" % name)
