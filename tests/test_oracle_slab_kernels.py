"""The oracle's z-slab PCG entry points (the block "device-scalar variants for the multi-GPU PCG" of include/manta_hip.h) against the
numpy statement of their contract in tests/slab_model.py, on the CPU: tests/test_gpu_slab_kernels.py then compares the HIP library
with an oracle that something independent has checked."""
import numpy as np
import pytest

import cases
import slab_model as sm
import util

TOL = 1e-5          # the project's bar for pressure (TOL of tests/test_gpu_parity.py)
# the two systems of the world runs: rows a multiple of 8 cells; 30 x 21 planes (2520 bytes: windows off the 16-byte grid), odd planes
WORLD_SYSTEMS = {"32x24x40": ((32, 24, 40), 3), "30x21x24": ((30, 21, 24), 5)}
# The bar on the true residual of a divided run is the undivided run's plus 1e-5 max|rhs| (max|rhs| is 1 here).  A converged run has a
# recursive residual below the accuracy, and its true residual differs from that by the fp32 drift of the recurrence (a few 1e-6 for
# pressures of order 1): with an accuracy of 5e-6 convergence implies the bar, a run that stops early or updates wrongly misses it.
WORLD_ACCURACY = 5e-6
WORLD_MAXITER = 100
_cache = {}


def world_system(name):
    if name not in _cache:
        dims, seed = WORLD_SYSTEMS[name]
        _cache[name] = sm.make_system(dims, seed)
    return _cache[name]


def world_run(impl, name, nranks, **kw):
    key = (impl.which, name, nranks, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = sm.run_world(impl, world_system(name), nranks, accuracy=WORLD_ACCURACY, max_iter=WORLD_MAXITER, **kw)
    return _cache[key]


@pytest.mark.parametrize("state", list(sm.STATES))
@pytest.mark.parametrize("world", sm.WORLDS)
def test_scalar_steps(oracle, world, state):
    """mf_cg_slab_alpha / mf_cg_slab_beta, every output bit for bit"""
    sm.check_scalar_steps(oracle, world, sm.STATES[state], "world %d %s" % (world, state))


def test_scalar_cases_reach_every_outcome():
    for world in sm.WORLDS:
        stops = {sm.expected_stop(norms) for _, _, norms in sm.scalar_cases(world)}
        assert stops == {0, 1, 2}, (world, stops)
    # the rank order of the sum matters where the issue asks for it
    for world in (3, 8):
        d = sm.ORDER_DOTS[world]
        assert sm.combine_rows(sm.rows([0] * world, d))[0] != sm.combine_rows(sm.rows([0] * world, d[::-1]))[0]


@pytest.mark.parametrize("state", list(sm.STATES))
@pytest.mark.parametrize("world", sm.WORLDS)
def test_composite_steps(oracle, world, state):
    """the same rows through mf_cg_slab_after_dp / mf_cg_slab_after_zr: scalar words 0-4 and 12, state, and the vector parts (inputs
    seeded with +-0, denormals and a few large values) bit for bit, signed zeros included"""
    ks = sm.kernel_system(oracle, (8, 6, 5), 2)
    XY = 8 * 6
    for i, (name, dots, norms) in enumerate(sm.scalar_cases(world)):
        g1 = sm.rows([0.0] * world, dots)
        g2 = sm.rows(norms, dots[::-1] if name.startswith("norm") else dots)
        sm.iteration_case(oracle, oracle, ks, world, g1, g2, 0.625, sm.STATES[state], sm.ACCURACY, 9, XY, 3 * XY, 40 + i,
                          "world %d %s %s" % (world, state, name))


@pytest.mark.parametrize("shape", ["n_own-0", "tail-1", "tail-2", "tail-3", "unaligned-30x21"])
def test_composite_steps_shapes(oracle, shape):
    dims, own_off, n_own = sm.SHAPES[shape]
    ks = sm.kernel_system(oracle, dims, 4)
    for state in ("state-null", "state-running"):
        sm.iteration_case(oracle, oracle, ks, 3, sm.rows([0, 0, 0], [1.0, 1e16, -1e16 + 4]), sm.rows([0.5, 0.1, 0.2], sm.ORDER_DOTS[3][::-1]),
                          0.625, sm.STATES[state], sm.ACCURACY, 2, own_off, n_own, 60, "%s %s" % (shape, state))


def test_orphaned_entries(oracle):
    sm.check_orphaned_entries(oracle, oracle)


@pytest.mark.parametrize("case", [c for c in sm.APPLY_CASES if not c.startswith("nt-")])
def test_apply_matrix_dot_dev(oracle, case):
    sm.check_apply_matrix_dot(oracle, oracle, case)


# ---- the one-process world ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WORLD_SYSTEMS))
@pytest.mark.parametrize("nranks", [1, 2, 3, 4])
def test_world_on_oracle(oracle, name, nranks):
    """nranks == 1 is mf_cg_solve on the undivided system (same iteration count, pressure within TOL); more ranks change the iterates
    (block-Jacobi preconditioner) and must converge to a true residual no larger than the undivided run's plus 1e-5 max|rhs|"""
    S = world_system(name)
    one = world_run(oracle, name, 1)
    pres, (it_b, res_b, _) = cases.run_cg_impl(oracle, S["dims"], S["flags"], S["A"], S["rhs"], 2, WORLD_ACCURACY, WORLD_MAXITER)
    assert 3 < it_b < WORLD_MAXITER
    w = world_run(oracle, name, nranks)
    print("%s nranks %d: %d iterations (mf_cg_solve %d), state %s, true residual %.3e" % (
        name, nranks, w["iters"], it_b, w["state"], sm.true_residual(S, w["pressure"])))
    assert 3 < w["iters"] < WORLD_MAXITER and w["state"] == [1, w["iters"]]
    if nranks == 1:
        assert w["iters"] == it_b
        print("   pressure bit-identical to mf_cg_solve: %s" % np.array_equal(w["pressure"].view(np.uint32), pres.view(np.uint32)))
        assert util.rel_err(w["pressure"], pres) <= TOL
        assert np.float32(w["scalars"][0][sm.RESNORM]) == np.float32(res_b)
    assert sm.true_residual(S, w["pressure"]) <= sm.true_residual(S, one["pressure"]) + 1e-5 * float(np.abs(S["rhs"]).max())


def test_world_y_cut_preconditioner(oracle):
    """one extra case: the preconditioner also cut into blocks of 8 rows along y"""
    S = world_system("32x24x40")
    one = world_run(oracle, "32x24x40", 1)
    w = world_run(oracle, "32x24x40", 2, blocking=(8, 0))
    assert 3 < w["iters"] < WORLD_MAXITER and w["state"] == [1, w["iters"]]
    assert sm.true_residual(S, w["pressure"]) <= sm.true_residual(S, one["pressure"]) + 1e-5 * float(np.abs(S["rhs"]).max())


def check_extra_is_noop(impl, name, nranks, extra, diverge_at):
    """iterations queued past the stop leave pressure, residual, state, sigma, beta and resNorm exactly as the stop left them"""
    base = world_run(impl, name, nranks, diverge_at=diverge_at)
    more = world_run(impl, name, nranks, diverge_at=diverge_at, extra=extra)
    assert more["queued"] == base["queued"] + extra and base["stopped_at"] == base["queued"]
    assert base["state"] == more["state"] and base["state"][0] == (2 if diverge_at else 1)
    if diverge_at:
        assert base["state"] == [2, diverge_at]
    sm.assert_bits(more["pressure"], base["pressure"], "pressure after %d more iterations" % extra)
    sm.assert_bits(more["residual"], base["residual"], "residual after %d more iterations" % extra)
    for w in (sm.SIGMA, sm.BETA, sm.RESNORM):
        sm.assert_bits(more["scalars"][:, w], base["scalars"][:, w], "scalar word %d" % w)
    # what the header says of a stopped alpha step
    assert (more["scalars"][:, sm.ALPHA].view(np.uint32) == 0).all() and (more["scalars"][:, sm.NALPHA].view(np.uint32) == 0x80000000).all()
    assert (more["scalars"].view(np.int32)[:, sm.XPENDING] == 0).all()


@pytest.mark.parametrize("stop", ["converged", "diverged"])
@pytest.mark.parametrize("extra", [1, 5])
@pytest.mark.parametrize("nranks", [1, 3])
@pytest.mark.parametrize("name", list(WORLD_SYSTEMS))
def test_iterations_queued_past_the_stop_are_noops(oracle, name, nranks, extra, stop):
    check_extra_is_noop(oracle, name, nranks, extra, 3 if stop == "diverged" else None)
