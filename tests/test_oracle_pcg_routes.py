"""Pins the oracle to the reference's compiled GridCg / ApplyMatrix / MIC on the inputs of tests/test_gpu_pcg_routes.py, which
uses the oracle as its yardstick: the route-table shapes, the solves stopped after k iterations, the liquid systems with incoming
values outside the fluid, and caller-built couplings across row and plane ends.  Bit-exact everywhere."""
import numpy as np
import pytest

import cases
import util
from util import assert_bitexact

pytestmark = pytest.mark.skipif(not util.have_ref(), reason="compiled reference (oracle/_ref) not present")


def _solve(run, *args, **kw):
    try:
        return run(*args, **kw)
    except RuntimeError as e:
        if "diverged" not in str(e):
            raise
        return None


def _same(got, want, what):
    if got is None or want is None:
        assert got is None and want is None, "%s: only one side diverged" % what
        return
    assert got[1][0] == want[1][0], "%s: iterations %s vs %s" % (what, got[1], want[1])
    assert_bitexact(got[0], want[0], what + ": dst")
    assert_bitexact(np.float32(got[1][1:]), np.float32(want[1][1:]), what + ": resNorm/sigma")


def _check(oracle, dims, flags, A, rhs, pc, acc, iters, l2=0, work=None, what=""):
    got = _solve(cases.run_cg_impl, oracle, dims, flags, A, rhs, pc, acc, iters, l2, work=work)
    want = _solve(cases.run_cg_ref, dims, flags, A, rhs, pc, acc, iters, l2, work=work)
    _same(got, want, what)
    return want


ROUTES = [pytest.param(d, pc, id="%dx%dx%d-pc%d" % (d + (pc,))) for d, _ in cases.PCG_ROUTES for pc in ((2, 0) if d[2] > 1 else (0,))]


@pytest.mark.parametrize("dims,pc", ROUTES)
@pytest.mark.parametrize("acc,iters", [(1e-9, 4), (1e-3, 400)], ids=["stopping", "converging"])
@pytest.mark.parametrize("l2", [0, 1])
def test_cg_route_shapes(oracle, dims, pc, acc, iters, l2):
    flags, A, _ = cases.system_inputs(dims, 5)
    rhs = cases.cg_rhs(dims, flags, 5)
    want = _check(oracle, dims, flags, A, rhs, pc, acc, iters, l2, what="%s pc %d" % (dims, pc))
    if acc > 1e-6:
        assert 0 < want[1][0] < iters, want[1]      # a converging case converges


@pytest.mark.parametrize("dims,pc", [((13, 11, 9), 2), ((16, 67, 5), 2), ((37, 29, 1), 0)])
def test_cg_stopped_after_k_iterations(oracle, dims, pc):
    flags, A, _ = cases.system_inputs(dims, 5)
    rhs = cases.cg_rhs(dims, flags, 5)
    for k in range(1, 13):
        _check(oracle, dims, flags, A, rhs, pc, 1e-7, k, what="%s after %d iterations" % (dims, k))


@pytest.mark.parametrize("dims,box,variant", [pytest.param(d, box, v, id="%dx%dx%d-%s" % (d + (v,)))
                                              for d, box, _ in cases.LIQUID_SHORTCUT for v in
                                              ("clean", "rhs_empty_bundle", "rhs_minus_zero", "tmp_empty_bundle", "tmp_beside_fluid",
                                               "search_nonfluid", "rhs_outside_xrange") if v != "rhs_outside_xrange" or box[1] + 9 < d[0]])
def test_cg_liquid_incoming_values(oracle, dims, box, variant):
    flags, A, rhs = cases.liquid_box_system(dims, box, 9)
    edit, work = cases.liquid_variants(dims, box, flags)[variant]
    rhs = rhs.copy()
    for cell, v in (edit or {}).items():
        rhs[cell] = v
    _check(oracle, dims, flags, A, rhs, 2, 1e-4, 30, 0, work, what="%s %s" % (dims, variant))


def test_cg_liquid_many_bundles(oracle):
    """the liquid case of test_gpu_pcg_routes sized for 256 CUs (17 x 17 bundles of rows)"""
    dims = (32, 136, 136)
    flags, A, rhs = cases.liquid_box_system(dims, (9, 20, 1, 68, 1, 135), 13)
    want = _check(oracle, dims, flags, A, rhs, 2, 1e-3, 60, what="%s liquid" % (dims,))
    assert 3 < want[1][0] < 60, want[1]


@pytest.mark.parametrize("dims,box", [pytest.param(d, box, id="%dx%dx%d" % d) for d, box, _ in cases.LIQUID_SHORTCUT])
def test_mic_apply_keeps_dst_outside_the_fluid(oracle, dims, box):
    sx, sy, sz = dims
    flags, A, _ = cases.liquid_box_system(dims, box, 9)
    var1 = util.rand_real((sz, sy, sx), 17)
    sentinel = np.float32(-7.25)
    f, dA = oracle.dev(flags), [oracle.dev(a) for a in A]
    ap = oracle.dev(np.zeros((sz, sy, sx), np.float32))
    oracle.call("mf_mic_init", sx, sy, sz, f, ap, *dA, None)
    dst = oracle.dev(np.full((sz, sy, sx), sentinel, np.float32))
    oracle.call("mf_mic_apply", sx, sy, sz, f, dst, oracle.dev(var1), ap, dA[1], dA[2], dA[3], None)
    ap_r = np.zeros((sz, sy, sx), np.float32)
    util.refcall("ref_mic_init", sx, sy, sz, flags, ap_r, *A)
    dst_r = np.full((sz, sy, sx), sentinel, np.float32)
    util.refcall("ref_mic_apply", sx, sy, sz, flags, dst_r, var1, ap_r, *A)
    assert_bitexact(oracle.host(ap), ap_r, "Aprecond")
    assert_bitexact(oracle.host(dst), dst_r, "MIC apply")
    nonfluid = (flags & util.FLUID) == 0
    assert (dst_r[nonfluid] == sentinel).all()


@pytest.mark.parametrize("dims,packed", [((16, 12, 6), False), ((16, 11, 7), False), ((260, 7, 4), False), ((16, 12, 6), True),
                                         ((24, 9, 5), True), ((16, 12, 1), False), ((20, 11, 1), False), ((13, 10, 6), False),
                                         ((13, 10, 1), False)])
def test_apply_matrix_grid_ends(oracle, dims, packed):
    flags, A, src = cases.apply_matrix_edge_inputs(dims, 3, packed)
    assert_bitexact(cases.run_apply_matrix_impl(oracle, dims, flags, A, src), cases.run_apply_matrix_ref(dims, flags, A, src), "ApplyMatrix")
