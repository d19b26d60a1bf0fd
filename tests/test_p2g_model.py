"""The numpy model of the particle->grid transfers (tests/p2g_model.py) against the oracle's serial scatter, and the construction of
the inputs that tests/test_gpu_p2g_atomic.py feeds to the fp32-atomic kernels.  No GPU.

The oracle adds the same fp32 terms in particle order, so
  * on the dyadic family (all partial sums exact) it must equal the model's exact sums bit for bit, raw and finished;
  * on the random family it must lie within gamma(k-1) * sum|term| + u |S| per entry, be 0 where k = 0 and the one term where k = 1.
That validates the model's terms, indices and clamps before any kernel is measured with it."""
import numpy as np
import pytest

import p2g_cases as C
import p2g_model as M
from util import assert_bitexact


def _exact32(sums, what):
    s = sums.S.astype(np.float32)
    assert (s.astype(np.float64) == sums.S).all(), what + ": an exact sum is not an fp32 number"
    return s


@pytest.mark.parametrize("name", C.DYADIC)
def test_dyadic_family_is_exact_and_equals_oracle(name):
    inp, o = C.get(name), C.oracle_outputs(name)
    mac = inp.mac
    # every term is a multiple of 2^-7 and A < 2^17: any fp32 partial sum has at most 24 significant bits
    for what, s in (("weight", mac["weight"]), ("vel", mac["vel"]), ("cell weight", inp.cell(3)["weight"]), ("cell values", inp.cell(3)["val"])):
        assert s.A.max() < 2.0 ** 17, (what, s.A.max())
        assert (np.round(s.S * 128) == s.S * 128).all() and s.min_term >= 2.0 ** -7, what
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


@pytest.mark.parametrize("name", C.RANDOM)
def test_random_family_oracle_within_bound(name):
    inp, o = C.get(name), C.oracle_outputs(name)
    mac = inp.mac
    for s in (mac["weight"], mac["vel"], inp.cell(3)["weight"], inp.cell(3)["val"], inp.cell(1)["val"]):
        assert s.min_term >= 2.0 ** -100        # no term that a flushing fp32 atomic would drop
    print(name, "used share of the bound: weight %.3f vel %.3f" % (
        C.check_sums(o["acc_weight"], mac["weight"], "raw MAC weight"), C.check_sums(o["acc_vel"], mac["vel"], "raw MAC vel")))
    C.check_quotients(o["vel"], mac["vel"], mac["weight"], None, "finished vel")
    assert_bitexact(o["velOld"], o["vel"], "velOld")
    *_, stomped, _ = M.quotient_classes(mac["vel"], mac["weight"])
    assert (o["weight"][stomped] == 0).all()
    assert C.left_out_share(mac["vel"], mac["weight"]) <= 0.05
    for nc in (1, 3):
        c = inp.cell(nc)
        C.check_sums(o["wtmp%d" % nc], c["weight"], "cell weight sums")
        den = c["weight"].tiled(nc)
        C.check_quotients(o["target%d" % nc], c["val"], den, 0.0, "target, ncomp %d" % nc)
        assert C.left_out_share(c["val"], den) <= 0.05
    assert (mac["weight"].k == 0).any()
    assert (mac["weight"].k == 1).any() or inp.dims[2] == 1      # in 2-D the two z corners alias: k is even
    if name == "crowded":
        assert mac["weight"].k.max() >= 3000      # the 6000-particle cell, less the excluded third


@pytest.mark.parametrize("m", [1, 7, 63, 65, 255, 257])
def test_prefixes_equal_oracle(m):
    """the partial-last-block inputs: the first m particles of the pattern input, with the stride of all of them"""
    inp, o = C.get("patterns").prefix(m), C.oracle_outputs("patterns", m)
    assert inp.np == m and C.get("patterns").np > 257
    assert_bitexact(o["acc_weight"], _exact32(inp.mac["weight"], "weight"), "raw MAC weight")
    assert_bitexact(o["acc_vel"], _exact32(inp.mac["vel"], "vel"), "raw MAC vel")


def test_plugins_equal_the_abi_on_the_oracle(oracle_backend):
    """the comparison the GPU test makes through the plugins, here with the oracle behind the package"""
    C.check_plugins_equal_abi(C.run_plugins(C.get("hits"), True), C.oracle_outputs("hits"))


def test_run_flip_pkg_restores_the_switch_when_it_raises(oracle_backend):
    import cases
    import util
    from mantaflow_amd import plugins
    inp = C.get("patterns")
    flags, vel = util.make_flags(*inp.dims, 7), util.rand_vel(*inp.dims, 8)
    with pytest.raises(RuntimeError):       # a particle-data array of the wrong length
        cases.run_flip_pkg(inp.dims, flags, vel, vel, inp.pos.copy(), inp.pflag.copy(), inp.pvel[:, :5].copy(), deterministic=False)
    assert plugins._deterministic_p2g is True


# ---- what each input is built to force -------------------------------------------------------------------------------------------
def test_table_load_per_block():
    """k_p2g_mac_lds: 2048 slots per block of 256 particles.  Cell-ordered inputs stay far below it (hits, short probe chains);
    shuffled ones on a grid of 3n >> 2048 exceed it, so contributions must overflow to global atomics by pigeonhole."""
    assert C.distinct_per_block("hits").max() <= 512
    for name in ("d3-shuffled", "r3"):
        inp = C.get(name)
        assert 3 * np.prod(inp.dims) > 50 * C.SLOTS
        assert C.distinct_per_block(name).max() > C.SLOTS, name
    # the cell-ordered bulk of d3 / d2 is far below the table size as well; d3's 500 scattered particles at the end are not
    d3, d2 = C.distinct_per_block("d3"), C.distinct_per_block("d2")
    assert np.median(d3) <= 1024 and d3.max() > C.SLOTS, (np.median(d3), d3.max())
    assert np.median(d2) <= 512, np.median(d2)


def test_run_patterns_present_for_every_component():
    """k_p2g_mac_atomic: all five run shapes occur in the keys of each of x, y and z, in both halves of a 16-lane DPP row"""
    inp = C.get("patterns")
    keys = inp.mac["keys"]
    for c in range(3):
        found = C.run_patterns(keys[c])
        for p in C.PATTERNS:
            assert found[p] == {0, 1}, ("component %d" % c, p, found[p])
    assert (keys[0] != keys[1]).any() and (keys[1] != keys[2]).any() and (keys[0] != keys[2]).any()
    # particle 0 is what inactive lanes read: active itself, with the largest value of the family
    assert keys[0, 0] >= 0 and (inp.pvel[:, 0] == 4).all()
    for m in (63, 65, 255, 257):
        assert (m + 1) % 8 == 0 or (m - 1) % 8 == 0


def test_inputs_cover_the_edges():
    for name in ("d3", "d2", "r3", "r2"):
        inp = C.get(name)
        sx, sy, sz = inp.dims
        act = M.active(inp.pflag, inp.ptype, C.EXCLUDE)
        assert (15000 if sz == 1 else 40000) < inp.np <= 170000
        assert (act & (inp.pos[0] < 0.5)).sum() >= 50 and (act & (inp.pos[0] >= sx - 1)).sum() >= 50
        assert 0.01 < ((inp.pflag & M.PDELETE) != 0).mean() < 0.03
        assert 0.25 < ((inp.ptype & C.EXCLUDE) != 0).mean() < 0.42
        if sz == 1:
            assert (inp.pos[2] < 1).all()
    for name, cells in (("d3", ((20, 8, 13), (21, 8, 13))), ("d2", ((40, 20, 0), (41, 20, 0))), ("hits", C.CROWDS_BIG[0][0:1] + C.CROWDS_BIG[1][0:1]),
                        ("crowded", ((7, 6, 5), (8, 6, 5)))):
        inp = C.get(name)
        c = inp.pos.astype(np.int64)
        for cell, least in zip(cells, (6000, 700)):
            assert ((c[0] == cell[0]) & (c[1] == cell[1]) & (c[2] == cell[2])).sum() >= least, (name, cell)


def test_run_pattern_detector():
    A, B, Cc, D = 5, 9, 11, 2
    f = C.run_patterns(np.array([A] * 8 + [A, A, B, B, Cc, Cc, D, D] + [A, B] * 4 + [A] * 8))
    assert f == {"eight_equal": {0, 1}, "AABBCCDD": {1}, "ABABABAB": {0}, "straddle": {0}, "split": set()}
    f = C.run_patterns(np.array([A, A, A, B, B, Cc, Cc, Cc, Cc, Cc, D, D, -1, D, A]))
    assert f["straddle"] == {0} and f["split"] == {1} and not f["eight_equal"] and not f["ABABABAB"]
