"""The geometry model of the ordered particle->grid path (tests/p2g_ordered_model.py) and the inputs that
tests/test_gpu_p2g_ordered.py feeds to csrc/p2g_ordered.hip (tests/p2g_ordered_cases.py).  No GPU.

  * the constants and comparisons the model mirrors are the kernel's (read from the sources as text);
  * the model's start / order, link distances, tile table and run shapes on hand-made examples;
  * every input reaches what it was planted for;
  * the oracle's serial scatter equals the sums of tests/p2g_model.py on every input: bit for bit on the dyadic family, within the
    bound of any fp32 summation order on the random one;
  * on the random family the order of summation shows: the oracle on the reversed particle order differs from the forward run in
    at least one node of every planted structure (a condition on the inputs -- the seeds are chosen so that it holds)."""
import os

import numpy as np
import pytest

import p2g_cases as C
import p2g_model as M
import p2g_ordered_cases as OC
import p2g_ordered_model as O
import util
from util import assert_bitexact

CSRC = os.path.join(util.ROOT, "mantaflow_amd", "csrc")


def test_constants_are_the_kernels():
    for fname, names in O.KERNEL_CONSTANTS.items():
        with open(os.path.join(CSRC, fname)) as f:
            found = O.constants_in(f.read())
        for name in names:
            assert name in found, "%s: no `constexpr int %s = ...`" % (fname, name)
            assert found[name] == getattr(O, name), "%s: %s is %d, the model has %d" % (fname, name, found[name], getattr(O, name))
    with open(os.path.join(CSRC, "p2g_ordered.hip")) as f:
        text = f.read()
    for line in O.KERNEL_PREDICATES:
        assert line in text, "p2g_ordered.hip no longer holds `%s`: the model's predicate for it may be stale" % line
    assert O.SCAN_BLOCK == 4096 and O.WAVE == O.GBLOCK and O.GX * O.GY * O.GZ == O.GBLOCK and O.WCAP <= 4095


def test_model_bin_order():
    n = 7
    keys = np.array([3, 7, 0, 3, 6, 7, 3, 0, 5, 3, 7, 6])          # 7 = n: skipped
    counts, start, order = O.bin_order(keys, n)
    assert counts.tolist() == [2, 0, 0, 4, 0, 1, 2] and start.tolist() == [0, 2, 2, 2, 6, 6, 7, 9]
    assert order.tolist() == [2, 7, 0, 3, 6, 9, 8, 4, 11]
    binned = np.nonzero(keys < n)[0]
    assert order.tolist() == binned[np.argsort(keys[binned], kind="stable")].tolist()
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 41, 3000)
    for a, b in zip(O.bin_order(keys, 40), O.bin_order_fast(keys, 40)):
        assert a.tolist() == b.tolist()
    assert [O.scan_blocks(v) for v in (4094, 4095, 4096, 8191)] == [1, 1, 2, 2]
    assert [O.sort_route(v) for v in (0, 1, 2, 32, 33, 4096, 4097)] == ["none", "none", "insertion", "insertion", "bitonic", "bitonic", "rank"]


def test_model_link_dists():
    # one cell; e along x: 0 1 1 0 1 1 1 1 1 1 1 0 -- entry 0 -> 3 (dist 3), entry 3 -> 11 (eight away: 7, walk finds a later one),
    # entry 1 -> 2 (1), entry 2 -> 4 (2), entry 10 -> none (0)
    ex = np.array([0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0])
    e = np.stack([ex, np.zeros_like(ex), 1 - ex], 0)
    order, dist, true, after = O.link_dists(np.zeros(12, np.int64), e, 1)
    assert order.tolist() == list(range(12)) and after.tolist() == list(range(11, -1, -1))
    assert dist[0].tolist() == [3, 1, 2, 7, 1, 1, 1, 1, 1, 1, 0, 0] and true[0].tolist() == [3, 1, 2, 8, 1, 1, 1, 1, 1, 1, 0, 0]
    assert dist[1].tolist() == [1] * 11 + [0] and (dist[2] == dist[0]).all()
    w = O.walk_outcomes(dist[0], true[0], after)
    assert np.nonzero(w["later"])[0].tolist() == [3] and not w["at7"].any() and not w["none"].any()
    ex = np.array([1] + [0] * 6 + [1] + [0] * 8)             # the seventh is the one; entry 7 has eight behind it and none with its bit
    _, dist, true, after = O.link_dists(np.zeros(16, np.int64), np.stack([ex, ex, ex], 0), 1)
    w = O.walk_outcomes(dist[0], true[0], after)
    assert np.nonzero(w["at7"])[0].tolist() == [0] and np.nonzero(w["none"])[0].tolist() == [7] and dist[0][7] == 0


def test_tile_table_hand_counted():
    """8 x 8 x 8, 2 x 2 x 2 tiles; cells (2,2,2): 5, (4,0,0): 7, (0,2,0): 3, (7,7,7): 2000"""
    dims = (8, 8, 8)
    counts = np.zeros(512, np.int64)
    for cell, c in (((2, 2, 2), 5), ((4, 0, 0), 7), ((0, 2, 0), 3), ((7, 7, 7), 2000)):
        counts[O.flat(dims, *cell)] = c
    t3, t0, t1 = (O.tile_table(dims, counts, m) for m in (3, 0, 1))
    assert len(t3) == 8
    assert t3[(0, 0, 0)] == (8, 5, "lds")            # cells 0..3 per axis: (2,2,2) and (0,2,0), in different rows
    assert t3[(1, 0, 0)] == (7, 7, "lds")            # x 3..7: (4,0,0) alone
    assert t0[(1, 0, 0)] == (12, 7, "lds")           # x 2..7: (2,2,2) as well
    assert t3[(0, 1, 0)] == (0, 0, "early")          # y 3..7: nothing
    assert t1[(0, 1, 0)] == (8, 5, "lds")            # y 2..7: (2,2,2) and (0,2,0)
    assert t3[(1, 1, 1)] == (2000, 2000, "fallback") and t0[(1, 1, 1)] == (2000, 2000, "fallback")
    assert t3[(0, 1, 1)] == (0, 0, "early")
    assert O.reach(0) == (2, 1, 1) and O.reach(2) == (1, 1, 2) and O.reach(3) == (1, 1, 1)
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 3, 512) * (rng.random(512) < 0.05)
    for mode in O.MODES:       # the early-out's row counts cover the cells of the table: `empty` never follows
        assert all(v[2] != "empty" for v in O.tile_table(dims, counts, mode).values())
    assert O.tile_info(np.full((8, 8, 8), 4), 3, (0, 0, 0))[0] == 4 * 64 and O.tile_info(np.full((8, 8, 8), 4), 3, (1, 1, 1))[0] == 4 * 125
    assert O.tiles_of((33, 7, 1)) == (3, 2, 1) and O.tiles_of((17, 11, 9)) == (5, 3, 3)


def test_run_shape_detector():
    n = 100
    A, B = 5, 9
    w0 = [A] * 64                                                     # run64; lane 63 | next lane 0 differ
    w1 = list(range(10, 74))                                          # runs1, and a run starting at lane 63
    w2 = [B] * 3 + [n] + [B] * 2 + [A] * 2 + [n] * 3 + [A] + list(range(20, 70)) + [B] * 2   # deleted_inside, skipped_run, end63
    w3 = [A] * 60 + [B] * 4                                           # lanes 255 | 256 share B
    w4 = [B] * 5 + [A] * 58 + [7]
    w5 = [7] * 3                                                      # cross_wave; partial
    keys = np.array(w0 + w1 + w2 + w3 + w4 + w5)
    assert [len(w) for w in (w0, w1, w2, w3, w4)] == [64] * 5
    f = O.run_shapes(keys, n)
    assert f == dict(run64=1, runs1=1, end63=1, start63=1, cross_wave=1, cross_block=1, deleted_inside=1, skipped_run=1, partial_wave=1), f
    assert O.run_shapes(np.array([A] * 128), n)["partial_wave"] == 0


def test_keys_and_e_bits():
    dims = (6, 5, 4)
    pos = np.array([[2.5, 2.75, 3.0, 3.25, 0.25, 5.9], [1.5, 1.5, 1.5, 1.5, 0.25, 4.9], [1.5, 1.5, 1.5, 1.5, 0.25, 3.9]], np.float32)
    pflag = np.array([0, 0, 0, M.PDELETE, 0, 0], np.int32)
    ptype = np.array([1, 4, 1, 1, 1, 1], np.int32)
    assert O.cell_keys(dims, pos, pflag, ptype, 4).tolist() == [O.flat(dims, 2, 1, 1), 120, O.flat(dims, 2, 1, 1), 120, 0, O.flat(dims, 4, 3, 2)]
    assert O.cell_keys(dims, pos, pflag).tolist()[1] == O.flat(dims, 2, 1, 1)
    assert O.e_bits(dims, pos)[0].tolist() == [0, 0, 1, 1, 0, 0]       # the last: the shifted index is clamped to sx - 2 as well
    assert O.apic_keys(dims, pos, pflag, ptype, 4, 0).tolist() == [O.flat(dims, 2, 1, 1), 120, O.flat(dims, 3, 1, 1), 120, 0, O.flat(dims, 5, 4, 3)]
    assert O.apic_keys(dims, pos, pflag, ptype, 4, 1)[2] == O.flat(dims, 2, 1, 1)


@pytest.mark.parametrize("name", OC.ALL_NAMES)
def test_input_reaches_what_it_was_planted_for(name):
    assert OC.reach(name)
    inp = OC.get(name)
    print(name, "particles", inp.np, "cells", inp.n)
    assert (name in OC.APIC_NAMES) == (inp.cp is not None)
    assert len(inp.regions) >= 1 and inp.family == name.rsplit("-", 1)[1]


def _exact32(sums, what):
    s = sums.S.astype(np.float32)
    assert (s.astype(np.float64) == sums.S).all(), what + ": an exact sum is not an fp32 number"
    return s


def _oracle_equals_model(inp, o):
    mac = inp.mac
    if inp.family == "dyadic":
        for what, s in (("weight", mac["weight"]), ("vel", mac["vel"]), ("cell weight", inp.cell(3)["weight"]), ("cell values", inp.cell(3)["val"])):
            assert s.A.max() < 2.0 ** 17, (what, s.A.max())
        w, v = _exact32(mac["weight"], "weight"), _exact32(mac["vel"], "vel")
        assert_bitexact(o["acc_weight"], w, "raw MAC weight")
        assert_bitexact(o["acc_vel"], v, "raw MAC vel")
        fv, fw = M.mac_finish(v, w)
        assert_bitexact(o["vel"], fv, "finished vel")
        assert_bitexact(o["velOld"], fv, "velOld")
        assert_bitexact(o["weight"], fw, "stomped weight")
        for nc in (1, 3):
            c = inp.cell(nc)
            cw = _exact32(c["weight"], "cell weight")
            assert_bitexact(o["wtmp%d" % nc], cw, "cell weight sums, ncomp %d" % nc)
            assert_bitexact(o["target%d" % nc], M.safe_div(_exact32(c["val"], "cell values"), cw, nc), "target, ncomp %d" % nc)
    else:
        C.check_sums(o["acc_weight"], mac["weight"], "raw MAC weight")
        C.check_sums(o["acc_vel"], mac["vel"], "raw MAC vel")
        C.check_quotients(o["vel"], mac["vel"], mac["weight"], None, "finished vel")
        assert_bitexact(o["velOld"], o["vel"], "velOld")
        for nc in (1, 3):
            c = inp.cell(nc)
            C.check_sums(o["wtmp%d" % nc], c["weight"], "cell weight sums")
            C.check_quotients(o["target%d" % nc], c["val"], c["weight"].tiled(nc), 0.0, "target, ncomp %d" % nc)


@pytest.mark.parametrize("name", OC.MAC_CELL_NAMES)
def test_oracle_equals_the_model_sums(name):
    _oracle_equals_model(OC.get(name), OC.oracle_outputs(name))


@pytest.mark.parametrize("m", OC.RUNS_PREFIXES)
def test_runs64_prefixes_equal_the_model_sums(m):
    inp = OC.get("runs64-dyadic")
    sub = inp.prefix(m)
    sub.family = "dyadic"
    _oracle_equals_model(sub, OC.oracle_outputs("runs64-dyadic", m))


@pytest.mark.parametrize("name", [n for n in OC.ALL_NAMES if n.endswith("-random")])
def test_order_of_summation_shows_in_every_structure(name):
    inp, apic = OC.get(name), name in OC.APIC_NAMES
    fwd, back = OC.oracle_outputs(name, None, apic), OC.oracle_outputs(name, None, apic, True)
    for r in inp.regions:
        if not r.order_shows:
            continue
        differ = 0
        for k in fwd:
            mask = inp.region_mask(r, fwd[k].size // inp.n)
            differ += int((util.bits(fwd[k])[mask] != util.bits(back[k])[mask]).sum())
        assert differ > 0, "%s: no node of `%s` depends on the particle order" % (name, r.label)
