"""Ties tests/golden/multigrid.npz (described at the top of tests/test_gpu_multigrid.py) to the compiled reference rather than to the
product: the reference's own solvePressure(preconditioner = PcMGDynamic) reproduces the recorded digests of the Dynamic cases bit for
bit.  Skipped where the compiled reference is not present."""
import hashlib

import numpy as np
import pytest

import mg_cases
import util

pytestmark = pytest.mark.skipif(not util.have_ref(), reason="compiled reference (oracle/_ref) not built")

# the two largest sizes take the single reference run of the GPU suite (test_gpu_multigrid.py checks the same digests there)
SIZES = [d for d in mg_cases.SIZES if d[0] * d[1] * d[2] <= 52 ** 3]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("dims", SIZES, ids=lambda d: "%dx%dx%d" % d)
@pytest.mark.parametrize("kind", list(mg_cases.KINDS))
def test_reference_reproduces_dynamic_cases(kind, dims):
    g = np.load(mg_cases.GOLDEN)
    flags, vel, phi, kw = mg_cases.inputs(kind, dims)
    name = mg_cases.case_name(kind, dims)
    r = mg_cases.run_ref(dims, flags, vel, phi, **kw)
    assert _sha(r["pressure"]) == bytes(g["sha_p__" + name]).hex(), name
    assert _sha(r["vel"]) == bytes(g["sha_v__" + name]).hex(), name


@pytest.mark.parametrize("acc", [1e-4, 1e-3])
def test_reference_reproduces_fractions_case(acc):
    g = np.load(mg_cases.GOLDEN)
    dims, flags, vel, fr = mg_cases.fractions_inputs_model()
    r = mg_cases.run_ref(dims, flags, vel, None, fractions=fr, cgAccuracy=acc)
    util.assert_bitexact(r["pressure"], g["fractions__%g__pressure" % acc], "fractions case pressure")
    assert _sha(r["vel"]) == bytes(g["fractions__%g__sha_v" % acc]).hex()


def test_mgsolve_first_step_is_a_dynamic_solve_of_the_reference():
    """the sequences run on one reference solver, which the shim cannot do; their first solves are plain Dynamic / first-Static solves"""
    g = np.load(mg_cases.GOLDEN)
    flags, vel, pc, kw = mg_cases.mgsolve_step(0, None)
    r = mg_cases.run_ref((52, 52, 52), flags, vel, None, **kw)
    assert _sha(r["pressure"]) == bytes(g["mgsolve__0__sha_p"]).hex()
    fa, va, kw = mg_cases.static_sequence()[0]
    r = mg_cases.run_ref(mg_cases.STATIC_DIMS, fa, va, None, **kw)
    assert _sha(r["pressure"]) == bytes(g["static__a__sha_p"]).hex()
