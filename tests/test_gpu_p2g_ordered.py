"""-m gpu: the ordered (default) particle->grid path kernel by kernel -- the binning of csrc/p2g_ordered.hip (k_bin_keys, the
three-launch scan, k_bin_place, k_bin_sort_cells, k_bin_sort_big, k_bin_payload, k_bin_links) and its gathers (k_gather,
k_gather_wave, k_gather_apic) -- through the C ABI with deterministic = 1, against the oracle's serial scatter, bit for bit.

Every input (tests/p2g_ordered_cases.py) plants one structure per region of the grid and first re-asserts, with the numpy model of
the geometry (tests/p2g_ordered_model.py), that it reaches the branch it was planted for; tests/test_p2g_ordered_model.py holds the
same predicates for a machine without a GPU.  Outputs start dirty, every input runs twice and the re-run must be bit-identical, and
a difference is reported with the structures its nodes belong to."""
import os
import subprocess
import sys

import numpy as np
import pytest

import p2g_cases as C
import p2g_ordered_cases as OC
from util import assert_bitexact

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "p2g_sequential_worker.py")


def _equals_oracle_twice(hip, name, entry, m=None):
    assert OC.reach(name)
    inp, o = OC.get(name), OC.oracle_outputs(name, m, entry == "apic")
    first, again = OC.run_entry(hip, inp, entry, m), OC.run_entry(hip, inp, entry, m)
    for k in first:
        OC.assert_same(inp, first[k], o[k], "%s: %s vs the serial scatter" % (entry, k))
        OC.assert_same(inp, again[k], first[k], "%s: %s, re-run" % (entry, k))
    return first


@pytest.mark.parametrize("entry", OC.ENTRIES)
@pytest.mark.parametrize("name", OC.MAC_CELL_NAMES)
def test_structure_bit_identical(hip, name, entry):
    """raw sums (mac_accum), finished vel / velOld / weight (mac), divided target and weight sums (grid1, grid3)"""
    _equals_oracle_twice(hip, name, entry)


@pytest.mark.parametrize("name", OC.APIC_NAMES)
def test_apic_bit_identical(hip, name):
    """k_gather_apic behind bin_particles with face keys: crowded faces (insertion, bitonic and rank-counting sort per component) and
    border particles"""
    _equals_oracle_twice(hip, name, "apic")


@pytest.mark.parametrize("entry", OC.ENTRIES)
@pytest.mark.parametrize("m", OC.RUNS_PREFIXES)
@pytest.mark.parametrize("family", OC.FAMILIES)
def test_runs64_prefixes(hip, family, m, entry):
    """the first m particles of the run-shape input with the stride of all of them: a last wave and a last block partly past np"""
    _equals_oracle_twice(hip, "runs64-" + family, entry, m)


@pytest.mark.parametrize("entry", ("mac", "grid3"))
def test_no_state_survives_a_smaller_call(hip, entry):
    """crowded cells, then 7 particles on another grid, then the crowded cells again in one process: the scratch slices are re-cut for
    the smaller np, and keys / nbig / the list of crowded cells of the first call must not reach the third"""
    big, small = OC.get("sorts-random"), OC.get("runs64-random")
    first = _equals_oracle_twice(hip, "sorts-random", entry)
    o = OC.oracle_outputs("runs64-random", 7)
    for k, v in OC.run_entry(hip, small, entry, 7).items():
        OC.assert_same(small, v, o[k], "%s: %s of the 7-particle call" % (entry, k))
    for k, v in OC.run_entry(hip, big, entry).items():
        OC.assert_same(big, v, first[k], "%s: %s of the third call vs the first" % (entry, k))


def test_sequential_kernels(hip, tmp_path):
    """k_p2g_mac_sequential / k_p2g_cell_sequential<1|3> (MF_P2G_SEQUENTIAL, read once per process) in a fresh child process"""
    out = str(tmp_path / "sequential.npz")
    env = dict(os.environ, MF_P2G_SEQUENTIAL="1")
    assert "MF_P2G_SEQUENTIAL" not in os.environ
    r = subprocess.run([sys.executable, WORKER, out], env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    assert "MF_P2G_SEQUENTIAL" not in os.environ
    got, o = np.load(out), C.oracle_outputs("patterns")
    for k in ("vel", "velOld", "weight", "target1", "wtmp1", "target3", "wtmp3"):
        assert_bitexact(got[k], o[k], "sequential kernels: " + k)
