"""-m gpu: the fp32-atomic particle->grid mode (deterministic = 0) kernel by kernel -- k_p2g_mac_lds, k_p2g_mac_atomic,
k_p2g_cell_atomic<1> / <3> of csrc/flip.hip -- through the C ABI, against the oracle's serial scatter and the numpy model
(tests/p2g_model.py).  tests/test_p2g_model.py validates the model and asserts, without a GPU, what each input is built to force
(table load per block, run shapes per component, A < 2^17, no denormal terms, left-out share).

  dyadic family   every partial sum of any order is exact in fp32, so the atomic kernels must equal the serial scatter BIT FOR BIT,
                  raw sums and finished vel / velOld / weight / target alike: a lost, doubled or misrouted contribution cannot hide
  random family   per entry |got - S| <= gamma(k-1) * sum|term| + u |S| (a theorem for any summation order, no margin), exactly 0
                  where k = 0, the one term where k = 1; divided outputs within the propagated bound where the weight sum is
                  >= 1e-3, exactly the stomped value where it is below 1e-6 in any order

k_p2g_mac_atomic is selected with MF_P2G_NOLDS, which the dispatcher reads at every call."""
import numpy as np
import pytest

import p2g_cases as C
import p2g_model as M
from util import assert_bitexact

pytestmark = pytest.mark.gpu

MAC_KERNELS = ("lds", "grouped")      # k_p2g_mac_lds ; k_p2g_mac_atomic (DPP-grouped runs)
PREFIXES = (1, 7, 63, 65, 255, 257)   # partial last block of 256; 8k +- 1 for the groups of 8 lanes


@pytest.fixture()
def select(monkeypatch):
    def f(kernel):
        if kernel == "grouped":
            monkeypatch.setenv("MF_P2G_NOLDS", "1")
        else:
            monkeypatch.delenv("MF_P2G_NOLDS", raising=False)
    return f


def _mac_equals_oracle(hip, name, m=None):
    o = C.oracle_outputs(name, m)
    inp = C.get(name)
    vel, w = C.run_mac_accum(hip, inp, m)
    assert_bitexact(w, o["acc_weight"], "raw weight sums")
    assert_bitexact(vel, o["acc_vel"], "raw vel sums")
    vel, velOld, w = C.run_mac(hip, inp, m)
    assert_bitexact(w, o["weight"], "stomped weight")
    assert_bitexact(vel, o["vel"], "finished vel")
    assert_bitexact(velOld, o["velOld"], "velOld")


# ---- (a) dyadic: exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.DYADIC)
@pytest.mark.parametrize("kernel", MAC_KERNELS)
def test_dyadic_mac_bit_identical(hip, select, kernel, name):
    """lds: `hits` stays in the table (<= 512 addresses per block), `d3-shuffled` overflows it (> 2048 per block: probe chains, then
    global atomics), d3 / d2 mix both; grouped: `patterns` holds every run shape for every component, the others long runs
    (cell-ordered), none (shuffled), the two aliasing z corners of 2-D, clamped border stencils, deleted and excluded particles"""
    select(kernel)
    if name == "hits":
        assert C.distinct_per_block(name).max() <= 512
    if name == "d3-shuffled":
        assert C.distinct_per_block(name).max() > C.SLOTS
    if name == "patterns":
        assert all(C.run_patterns(k)[p] == {0, 1} for k in C.get(name).mac["keys"] for p in C.PATTERNS)
    _mac_equals_oracle(hip, name)


@pytest.mark.parametrize("m", PREFIXES)
@pytest.mark.parametrize("kernel", MAC_KERNELS)
def test_dyadic_mac_partial_block(hip, select, kernel, m):
    select(kernel)
    assert C.get("patterns").prefix(m).np == m
    _mac_equals_oracle(hip, "patterns", m)


@pytest.mark.parametrize("name", ("d3", "d3-shuffled", "d2-shuffled", "hits", "patterns"))
@pytest.mark.parametrize("ncomp", (1, 3))
def test_dyadic_cell_bit_identical(hip, ncomp, name):
    o = C.oracle_outputs(name)
    tgt, w = C.run_cell(hip, C.get(name), ncomp)
    assert_bitexact(w, o["wtmp%d" % ncomp], "weight sums")
    assert_bitexact(tgt, o["target%d" % ncomp], "target")


@pytest.mark.parametrize("m", (1, 7, 255, 257))
@pytest.mark.parametrize("ncomp", (1, 3))
def test_dyadic_cell_partial_block(hip, ncomp, m):
    o = C.oracle_outputs("patterns", m)
    tgt, w = C.run_cell(hip, C.get("patterns"), ncomp, m)
    assert_bitexact(w, o["wtmp%d" % ncomp], "weight sums")
    assert_bitexact(tgt, o["target%d" % ncomp], "target")


# ---- (b) random: the bound, entry by entry ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.RANDOM)
@pytest.mark.parametrize("kernel", MAC_KERNELS)
def test_random_mac_within_bound(hip, select, kernel, name):
    select(kernel)
    inp = C.get(name)
    mac = inp.mac
    assert min(mac["weight"].min_term, mac["vel"].min_term) >= 2.0 ** -100
    vel, w = C.run_mac_accum(hip, inp)
    print("%s %s: used share of the bound, weight %.3f vel %.3f" % (
        kernel, name, C.check_sums(w, mac["weight"], "raw weight sums"), C.check_sums(vel, mac["vel"], "raw vel sums")))
    vel, velOld, w = C.run_mac(hip, inp)
    C.check_quotients(vel, mac["vel"], mac["weight"], None, "finished vel")
    assert_bitexact(velOld, vel, "velOld")
    _, _, divided, stomped, _ = M.quotient_classes(mac["vel"], mac["weight"])
    assert (w[stomped] == 0).all(), "a weight below 1e-6 was not stomped"
    assert (np.abs(w.astype(np.float64) - mac["weight"].S)[divided] <= mac["weight"].bound[divided]).all(), "finished weight"
    assert C.left_out_share(mac["vel"], mac["weight"]) <= 0.05


@pytest.mark.parametrize("name", C.RANDOM)
@pytest.mark.parametrize("ncomp", (1, 3))
def test_random_cell_within_bound(hip, ncomp, name):
    inp = C.get(name)
    c = inp.cell(ncomp)
    assert min(c["weight"].min_term, c["val"].min_term) >= 2.0 ** -100
    tgt, w = C.run_cell(hip, inp, ncomp)
    print("ncomp %d %s: used share of the bound, weight %.3f" % (ncomp, name, C.check_sums(w, c["weight"], "weight sums")))
    den = c["weight"].tiled(ncomp)
    C.check_quotients(tgt, c["val"], den, 0.0, "target")
    assert C.left_out_share(c["val"], den) <= 0.05


# ---- (c) through the plugins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("d3-shuffled", "d2", "hits"))
def test_plugins_atomic_mode_equals_ordered_mode(hip_backend, name):
    """mapPartsToMAC / mapPartsToGrid / mapPartsToGridVec3 on exactly summable inputs: setDeterministicP2G(False) == (True) bit for
    bit, a re-run equals itself, both equal the serial scatter; the switch is back at its default afterwards"""
    from mantaflow_amd import plugins
    inp = C.get(name)
    try:
        a = C.run_plugins(inp, False)
        assert plugins._deterministic_p2g is True
        a2 = C.run_plugins(inp, False)
        b = C.run_plugins(inp, True)
    finally:
        plugins.setDeterministicP2G(True)
    for k in C.P2G_KEYS:
        assert_bitexact(a[k], b[k], k + ": atomic vs ordered")
        assert_bitexact(a[k], a2[k], k + ": re-run")
    C.check_plugins_equal_abi(a, C.oracle_outputs(name))
