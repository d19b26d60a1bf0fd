"""CPU: the numpy model of the two smooth particle level sets (tests/partls_model.py) against tests/golden/partls.npz, bit for bit and
with no exemption.  The fixture holds the outputs of the reference itself (zoharl3/mantaflow, plugin/flip.cpp:365-581), recorded by
tools/record_partls.py with one OpenMP thread; its inputs are regenerated here from the model's seeded generators:

  <case>/phi      averagedParticleLevelset (avg/*) or improvedParticleLevelset (imp/*) with the case's arguments
  <case>/stage    improved cases with smoothing: the same call with smoothen = smoothenNeg = 0

The cases are the smallest that reach every path: r = 1, 2, 3 (at 12x10x9 with r = 3 the neighbourhood leaves the grid from every
cell), 3-D and 2-D, every (smoothen, smoothenNeg) pair of the issue, both clamps of the correction, the three branches of the
eigenvalue routine, a weight sum in (0, 1e-6], a particle on a cell centre, deleted / out-of-domain / excluded particles, and the
empty particle system."""
import os

import numpy as np
import pytest

import partls_model as M
import util

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partls.npz"))


@pytest.mark.parametrize("name", list(M.CASES))
def test_model_equals_the_reference(name):
    phi, stage, info, _ = M.model_case(name)
    util.assert_bitexact(phi, GOLDEN[name + "/phi"], name + "/phi")
    if name + "/stage" in GOLDEN.files:
        util.assert_bitexact(stage, GOLDEN[name + "/stage"], name + "/stage")


def test_every_case_is_recorded():
    want = {n + "/phi" for n in M.CASES} | {n + "/stage" for n, c in M.CASES.items() if c["improved"] and (c["smoothen"] or c["smoothenNeg"])}
    have = {k for k in GOLDEN.files if not k.startswith("loop_")}
    assert want == have
    for name in M.LOOPS:
        assert GOLDEN[name + "/iters"].shape == (M.LOOP_STEPS,) and GOLDEN[name + "/crc"].shape == (M.LOOP_STEPS,)
        assert GOLDEN[name + "/phi"].shape == (M.LOOP_RES,) * 3


def test_the_fixture_reaches_every_path():
    tot = {}
    for name in M.CASES:
        for k, v in M.model_case(name)[2].items():
            tot[k] = tot.get(k, 0) + v
    # the three branches of the eigenvalue routine, and a correction below one
    assert tot["pos"] > 0 and tot["zero"] > 0 and tot["neg"] > 0 and tot["below_one"] > 0, tot
    # both clamps bind (t_low, t_high = 0.9, 1.2)
    assert tot["clamp0"] > 0 and tot["clamp1"] > 0, tot
    # a cell whose weights sum to something in (0, 1e-6]
    assert tot["tiny"] > 0, tot
    # the exact lattice is what makes h == 0
    assert M.model_case("imp/b3_r1_j00_s00")[2]["zero"] > 0
    # the set of (smoothen, smoothenNeg) pairs and of stencil radii
    pairs = {(c["smoothen"], c["smoothenNeg"]) for c in M.CASES.values()}
    assert {(0, 0), (1, 1), (2, 0), (0, 2), (3, 1), (1, 3)} <= pairs
    radii = {(M.radius_of(c["dims"], c["radiusFactor"])[1], c["dims"][2] > 1) for c in M.CASES.values()}
    assert {(1, True), (2, True), (3, True), (1, False), (2, False)} <= radii
    print("branch counts over the fixture:", tot)


def test_special_particles():
    # the particle on a cell centre: the distance of that cell to it is exactly 0, so its weight there is 1
    I = M.case_inputs("avg/b3_r1_j05_s11")
    frac = I["pos"] - np.floor(I["pos"])
    assert ((frac == 0.5).all(axis=1) & (I["pflag"] == 0)).any()
    assert (I["pflag"] & M.PDELETE).any()
    sx, sy, sz = M.B3
    assert ((I["pos"] < -1) | (I["pos"] >= np.array([sx, sy, sz]))).any()
    # the excluded particles change the result
    a = M.model_case("avg/b3_r1_j05_s00_ptype")[0]
    c = M.CASES["avg/b3_r1_j05_s00_ptype"]
    b, _ = M.particle_levelset(c["dims"], I["pos"], I["pflag"], False, **M.case_kwargs("avg/b3_r1_j05_s00_ptype"))
    assert not np.array_equal(a, b)


def test_empty_particle_system():
    # without smoothing: the radius inside, 0.5 on the border, exactly (the smoothing passes of the other two empty cases average
    # the radius with the zero border of their temporary grid; the model test above covers them)
    name = "avg/s2_empty_s00"
    c = M.CASES[name]
    want = np.full(c["dims"][::-1], M.radius_of(c["dims"], c["radiusFactor"])[0], np.float32)
    M.set_bound(want, np.float32(0.5))
    util.assert_bitexact(GOLDEN[name + "/phi"], want, name)
    for name in ("avg/s3_empty_s11", "imp/s2_empty_s11"):
        c = M.CASES[name]
        g = GOLDEN[name + "/phi"]
        assert np.isfinite(g).all() and abs(float(g[g.shape[0] // 2, 5, 5]) - float(M.radius_of(c["dims"], c["radiusFactor"])[0])) < 1e-6


def test_the_file_is_small():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(here, "partls.npz")) <= os.path.getsize(os.path.join(here, "nbflip.npz"))
