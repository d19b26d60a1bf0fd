"""The inputs of tests/test_gpu_base_edges.py, proven on the CPU: each builder of cases.py's edge section reaches the branches it
was planted for (numpy predicates on the inputs, at least 8 hits each; the isolated-cell patterns at least 1), and every case runs
through the package on the oracle backend without raising and with finite results.  The particles planted beside the domain for
advectInGrid are checked against the documented rule (the flag of the nearest cell decides; cases.clamp_bisect_model)."""
import numpy as np
import pytest

import cases
import util


def _finite(out, what):
    for k, v in (out.items() if isinstance(out, dict) else [("", out)]):
        if isinstance(v, np.ndarray) and v.dtype.kind == "f":
            assert np.isfinite(v).all(), "%s %s: not finite" % (what, k)


@pytest.mark.parametrize("dims", cases.EDGE_DIMS)
def test_advect_parts_edge_inputs(oracle_backend, dims):
    I = cases.advect_parts_edge_inputs(dims, 19)
    cases.assert_reach(cases.advect_parts_edge_reach(dims, I), "advect_parts_edge_inputs%s" % (dims,))
    lim = max(dims) + 3.0
    assert np.isfinite(I["pos"]).all() and I["pos"].min() > -3.0 and I["pos"].max() < lim
    moved = 0
    for mode, dele, stop, skip in cases.ADVECT_PARTS_MODES:
        p, f = cases.run_advect_parts_edge(dims, I, mode, dele, stop, skip)
        _finite(p, "advectInGrid %s" % ((mode, dele, stop, skip),))
        if not dele and stop:
            cases.check_planted_against_model(I, p, f)
            moved += int((p[:, I["planted"]] != I["pos"][:, I["planted"]]).any(0).sum())
    assert moved >= 8      # the planted particles whose nearest cell is fluid are pulled towards the domain


@pytest.mark.parametrize("dims", cases.EDGE_DIMS)
def test_flip_edge_inputs(oracle_backend, dims):
    I = cases.flip_edge_inputs(dims, 14)
    cases.assert_reach(cases.flip_edge_reach(dims, I), "flip_edge_inputs%s" % (dims,))
    _finite(cases.run_flip_pkg(dims, I["flags"], I["vel"], I["velOld"], I["pos"], I["pflag"], I["pvel"], I["ptype"], 4), "flip transfers")


@pytest.mark.parametrize("dims", cases.EDGE_DIMS)
def test_surface_edge_inputs(oracle_backend, dims):
    I = cases.surface_edge_inputs(dims, 51)
    cases.assert_reach(cases.surface_edge_reach(dims, I), "surface_edge_inputs%s" % (dims,))
    out = cases.run_surface_pkg(dims, I)
    _finite(out, "surface pieces")
    prj = cases.run_project_pkg(dims, I)["project_XyZ"]
    live = (I["pflag"] & cases.PDELETE) == 0
    assert (prj[0, live] <= dims[0] - 2.5).all() and (prj[1, live] >= 2.5).all() and (prj[0, live] < 2.5).sum() >= 8     # "XyZ": x is not lifted
    # the planted cells do what they were planted for: exact distances in the union level set, untouched / pushed particles
    ci, cj, ck = cases.SURF_PATCH_ZERO
    inb, c = cases._cells_of(dims, I["pos"])
    alive = ((I["pflag"] & cases.PDELETE) == 0) & ((I["ptype"] & 4) == 0) & inb
    zero = alive & (c[0] == ci) & (c[1] == cj) & (c[2] == (ck if dims[2] > 1 else 0))
    assert (out["push"][:, zero] == I["pos"][:, zero]).all()                       # zero gradient: not pushed
    ci, cj, ck = cases.SURF_PATCH_UNIT
    unit = alive & (c[0] == ci) & (c[1] == cj) & (c[2] == (ck if dims[2] > 1 else 0))
    assert (out["push"][0, unit] > I["pos"][0, unit]).all() and (out["push"][1:, unit] == I["pos"][1:, unit]).all()   # pushed along +x only
    iso = cases.isolated_pattern_counts(I["fiso"])
    assert ((out["isolated"] != I["fiso"]).sum()) == iso["none"]


@pytest.mark.parametrize("dims", cases.EDGE_DIMS)
def test_markfluid_edge_inputs(oracle_backend, dims):
    I = cases.markfluid_edge_inputs(dims, 31)
    cases.assert_reach(cases.markfluid_edge_reach(dims, I), "markfluid_edge_inputs%s" % (dims,))
    out = cases.run_markfluid_pkg(dims, I)
    assert (out["flags_phi"] != out["flags"]).sum() >= 8


@pytest.mark.parametrize("dims,small", [((20, 14, 12), (10, 7, 6)), (cases.SIZE_2D, (12, 9, 1)), ((17, 11, 9), (9, 6, 5))])
def test_turb_edge_inputs(oracle_backend, dims, small):
    I = cases.turb_edge_inputs(dims, small, 91)
    cases.assert_reach(cases.turb_edge_reach(dims, I), "turb_edge_inputs%s" % (dims,))
    cases.assert_reach(cases.turb_clamp_reach(cases.run_turb_edge_pkg, dims, I), "noise clamp %s" % (dims,))
    _finite(cases.run_turb_edge_pkg(dims, I), "turbulence pieces")


@pytest.mark.parametrize("dims", [(14, 12, 10), cases.SIZE_2D])
def test_outflow_timestep_above_one(oracle_backend, dims):
    """applyOutflowBC with 4 * dt > 1 (timeStep = 3.6): there are outflow cells, and the step changes them"""
    sx, sy, sz = dims
    flags, vel = cases.advect_inputs(dims, 9, vmax=2.5, outflow=True)
    assert ((flags & util.OUTFLOW) != 0).sum() >= 8 and 4 * 0.9 > 1
    field = util.rand_vel(sx, sy, sz, 10)
    for order in (1, 2):
        _finite(cases.run_advect_pkg(dims, 0.9, flags, vel, field, 2, order=order), "MAC advection with outflow")


@pytest.mark.parametrize("dims", [(14, 12, 10), cases.SIZE_2D])
def test_outflow_edge_inputs(oracle_backend, dims):
    flags, vel, field = cases.outflow_edge_inputs(dims, 9)
    cases.assert_reach(cases.outflow_edge_reach(dims, flags), "outflow_edge_inputs%s" % (dims,))
    assert 4 * cases.OUTFLOW_DTS[0] > 1 > 4 * cases.OUTFLOW_DTS[1]
    for dt in cases.OUTFLOW_DTS:
        for order in (1, 2):
            _finite(cases.run_advect_pkg(dims, dt, flags, vel, field, 2, order=order), "MAC advection with outflow on both sides")


def test_sanitizer_program_runs_the_zmarch_shapes():
    """tools/zmarch_bounds.c (the oracle under AddressSanitizer / UBSan, a stand-alone program) carries the shape list of the GPU test"""
    import os
    import re
    src = open(os.path.join(util.ROOT, "tools", "zmarch_bounds.c")).read()
    body = re.search(r"SHAPES\[\]\[3\] = \{(.*?)\};", src, re.S).group(1)
    assert [tuple(int(v) for v in m) for m in re.findall(r"\{(\d+), (\d+), (\d+)\}", body)] == cases.ZMARCH_DIMS


@pytest.mark.parametrize("dims", [(14, 12, 10), cases.SIZE_2D])
def test_poisoned_pool_is_handed_out(oracle_backend, dims):
    """the poisoned tensors are the ones advectSemiLagrange works on, and nothing of them shows in the result"""
    sx, sy, sz = dims
    for kind, order, cm, ot, os_ in cases.ADVECT_POISON_CASES:
        flags, vel = cases.advect_inputs(dims, 9, vmax=2.5, outflow=(kind == 2))
        field = util.rand_real((sz, sy, sx), 10) if kind == 0 else util.rand_vel(sx, sy, sz, 10)
        kw = dict(order=order, clampMode=cm, orderTrace=ot, orderSpace=os_, strength=0.8 if order == 2 else 1.0)
        want = cases.run_advect_pkg(dims, 0.9, flags, vel, field, kind, **kw)
        got, seen = cases.run_advect_poisoned(dims, 0.9, flags, vel, field, kind, **kw)
        cases.check_poison_used(seen, kind, order)
        assert not np.isnan(got).any()
        util.assert_bitexact(got, want, "advectSemiLagrange from a poisoned pool %s" % ((kind, order, cm, ot, os_),))


@pytest.mark.parametrize("dims", cases.ZMARCH_DIMS)
def test_zmarch_depths_on_the_oracle(oracle_backend, dims):
    sx, sy, sz = dims
    flags, vel = cases.advect_inputs(dims, 9, vmax=2.5)
    for kind in (0, 1):
        field = util.rand_real((sz, sy, sx), 10) if kind == 0 else util.rand_vel(sx, sy, sz, 10)
        for order in (1, 2):
            want = cases.run_advect_pkg(dims, 0.9, flags, vel, field, kind, order=order)
            got, seen = cases.run_advect_poisoned(dims, 0.9, flags, vel, field, kind, order=order)
            cases.check_poison_used(seen, kind, order)
            util.assert_bitexact(got, want, "advectSemiLagrange %s kind %d order %d" % (dims, kind, order))
            # the border is what a cleared temp grid holds
            b = np.ones(got.shape[-3:], bool)
            b[(slice(1, -1),) * 3] = False
            assert (got[..., b] == 0).all()
