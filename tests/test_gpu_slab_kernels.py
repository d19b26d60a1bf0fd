"""-m gpu: the z-slab PCG entry points of the HIP library (the block "device-scalar variants for the multi-GPU PCG" of
include/manta_hip.h), one entry point per call on identical inputs, against the oracle and the numpy model of tests/slab_model.py
(tests/test_oracle_slab_kernels.py pins the oracle to that model on the CPU).

Element-wise results (residual, x, search, dst of the ApplyMatrix, tmp after the MIC apply) bit for bit; max-abs results, scalar words
and state exactly; dots within 2 n 2^-53 sum |p_i| of the exactly rounded sum of the same fp32 products (HIP sums its fp64 partials
in another order than a serial loop).  After a stop only what the header specifies is compared: x, residual, state, sigma, beta,
resNorm unchanged, alpha == 0, nalpha == -0, xpending == 0.  The test ids name the branch of pressure.hip a case takes."""
import numpy as np
import pytest

import slab_model as sm
import test_oracle_slab_kernels as cpu
import util

pytestmark = pytest.mark.gpu

# state on entry -> the branch of mf_cg_slab_after_dp / _after_zr it selects on the aligned shape
STATE_BRANCH = {"aligned-fused-with-state": "state-running", "aligned-state-null-one-thread-kernels": "state-null",
                "entered-stopped-state-1": "state-converged", "entered-stopped-state-2": "state-diverged"}


def both(oracle, hip, ks, world, g1, g2, state, own_off, n_own, seed, what, it=9):
    """the case on the HIP library and on the oracle, each against the model, and the two against each other where specified"""
    ha, hb = sm.iteration_case(oracle, hip, ks, world, g1, g2, 0.625, state, sm.ACCURACY, it, own_off, n_own, seed, what + " [hip]")
    oa, ob = sm.iteration_case(oracle, oracle, ks, world, g1, g2, 0.625, state, sm.ACCURACY, it, own_off, n_own, seed, what + " [oracle]")
    sm.assert_bits(ha["residual"], oa["residual"], what + ": residual hip vs oracle")
    sm.assert_bits(hb["x"], ob["x"], what + ": x hip vs oracle")
    sm.check_scalars(hb["sc"], ob["sc"], what + ": hip vs oracle")
    if not sm.stopped(state):
        sm.assert_bits(ha["tmp"], oa["tmp"], what + ": tmp hip vs oracle")
        assert ha["maxabs"] == oa["maxabs"] or n_own == 0
        if not sm.stopped(hb["state"]):
            sm.assert_bits(hb["search"], ob["search"], what + ": search hip vs oracle")
    return hb


@pytest.mark.parametrize("state", list(sm.STATES))
@pytest.mark.parametrize("world", sm.WORLDS, ids=lambda w: "world-%d" % w)
def test_scalar_steps(hip, world, state):
    """mf_cg_slab_alpha / mf_cg_slab_beta (one-thread kernels), every output bit for bit against the model"""
    sm.check_scalar_steps(hip, world, sm.STATES[state], "world %d %s" % (world, state))


@pytest.mark.parametrize("branch", list(STATE_BRANCH))
@pytest.mark.parametrize("world", sm.WORLDS, ids=lambda w: "world-%d" % w)
def test_after_dp_after_zr_scalar_cases(hip, oracle, world, branch):
    """every case of slab_model.scalar_cases (rank-order-sensitive sums, alpha = 0, norms at and around the accuracy and 1e35, NaN rows:
    converging and diverging in this very call among them) through the composite entry points on owned cells on the 16-byte grid"""
    state = sm.STATES[STATE_BRANCH[branch]]
    dims, own_off, n_own = sm.SHAPES["aligned"]
    ks = sm.kernel_system(oracle, dims, 2)
    seen = set()
    for i, (name, dots, norms) in enumerate(sm.scalar_cases(world)):
        g1 = sm.rows([0.0] * world, dots)
        g2 = sm.rows(norms, dots[::-1] if name.startswith("norm") else dots)
        hb = both(oracle, hip, ks, world, g1, g2, state, own_off, n_own, 40 + i, "%s world %d %s" % (branch, world, name))
        if hb["state"] is not None:
            seen.add(int(hb["state"][0]))
    if branch == "aligned-fused-with-state":
        assert seen == {0, 1, 2}, "the cases must run on, converge and diverge in this call: %s" % seen


@pytest.mark.parametrize("stop", ["converging-in-this-call", "diverging-fabricated-row-in-this-call", "alpha-zero-dp-sum-zero"])
@pytest.mark.parametrize("shape", ["aligned", "unaligned-30x21", "tail-3"])
def test_after_dp_after_zr_stop_in_this_call(hip, oracle, shape, stop):
    dims, own_off, n_own = sm.SHAPES[shape]
    ks = sm.kernel_system(oracle, dims, 4)
    dots = sm.ORDER_DOTS[3]
    g1 = sm.rows([0, 0, 0], [1.0, -1.0, 0.0] if stop.startswith("alpha") else [1.0, 1e16, -1e16 + 4])
    norms = {"c": [1e-5, 2e-4, 1e-7], "d": [0.5, 1e36, 0.1], "a": [0.5, 0.1, 0.2]}[stop[0]]
    hb = both(oracle, hip, ks, 3, g1, sm.rows(norms, dots[::-1]), (0, 0), own_off, n_own, 70, "%s %s" % (shape, stop), it=6)
    assert [int(v) for v in hb["state"]] == {"c": [1, 6], "d": [2, 6], "a": [0, 0]}[stop[0]]
    if stop.startswith("alpha"):
        assert hb["sc"][sm.ALPHA].view(np.uint32) == 0 and hb["sc"][sm.NALPHA].view(np.uint32) == 0x80000000


@pytest.mark.parametrize("state", ["with-state", "state-null", "entered-stopped-state-1", "entered-stopped-state-2"])
@pytest.mark.parametrize("shape", ["unaligned-30x21", "n_own-0", "tail-1", "tail-2", "tail-3"])
def test_after_dp_after_zr_shapes(hip, oracle, shape, state):
    """own_off * 4 % 16 != 0 (the unfused sequence), n_own == 0, and n_own % 4 in {1, 2, 3} with own_off = 0 (the scalar tails in
    block 0 of the fused kernels; with state == NULL the scalar search update).  Entered stopped, the unfused sequence once formed
    residual + (-0) * tmp: a -0 of the residual became +0 (and a cell whose tmp had overflowed NaN); it now returns on `done`."""
    dims, own_off, n_own = sm.SHAPES[shape]
    ks = sm.kernel_system(oracle, dims, 4)
    st = {"with-state": (0, 0), "state-null": None, "entered-stopped-state-1": (1, 3), "entered-stopped-state-2": (2, 5)}[state]
    both(oracle, hip, ks, 3, sm.rows([0, 0, 0], [1.0, 1e16, -1e16 + 4]), sm.rows([0.5, 0.1, 0.2], sm.ORDER_DOTS[3][::-1]),
         st, own_off, n_own, 60, "%s %s" % (shape, state), it=2)


def test_above_PCG_NT_CELLS_nt_branch(hip, oracle):
    """256 x 256 x 168 (11.0 Mi cells, 166 owned planes = 10.4 Mi cells > PCG_NT_CELLS): the non-temporal form of k_slab_axpy_r /
    k_slab_update_search_x and of the ranged dot of mf_apply_matrix_dot_dev.  The one parametrisation of this size."""
    dims = (256, 256, 168)
    XY = 256 * 256
    ks = sm.kernel_system(oracle, dims, 6)
    assert 166 * XY > 10 << 20
    both(oracle, hip, ks, 3, sm.rows([0, 0, 0], [1.0, 1e16, -1e16 + 4]), sm.rows([0.5, 0.1, 0.2], sm.ORDER_DOTS[3][::-1]),
         (0, 0), XY, 166 * XY, 80, "nt-1 256x256x168", it=2)
    sm.check_apply_matrix_dot(oracle, hip, "nt-256x256x168-packed-with-A0")


@pytest.mark.parametrize("case", [c for c in sm.APPLY_CASES if not c.startswith("nt-")])
def test_apply_matrix_dot_dev(hip, oracle, case):
    sm.check_apply_matrix_dot(oracle, hip, case)


def test_orphaned_entries(hip, oracle):
    """mf_cg_slab_alpha, mf_cg_slab_axpy2 (aligned: fused kernel; unaligned: the unfused sequence), mf_grid_scaled_add_dev with
    sign = +-1, mf_update_search_vec_dev, mf_grid_max_abs_dev, mf_grid_max_abs_dev_f64, mf_grid_dot_dev"""
    sm.check_orphaned_entries(oracle, hip)


# ---- the one-process world on the device -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cpu.WORLD_SYSTEMS))
@pytest.mark.parametrize("nranks", [1, 2, 3, 4], ids=lambda n: "nranks-%d" % n)
def test_world_on_hip(hip, oracle, name, nranks):
    S = cpu.world_system(name)
    want, got = cpu.world_run(oracle, name, nranks), cpu.world_run(hip, name, nranks)
    rg, rw = sm.true_residual(S, got["pressure"]), sm.true_residual(S, want["pressure"])
    print("%s nranks %d: iterations %d (oracle %d), state %s, rel err %.3e, true residual %.3e (oracle %.3e)" % (
        name, nranks, got["iters"], want["iters"], got["state"], util.rel_err(got["pressure"], want["pressure"]), rg, rw))
    assert got["iters"] == want["iters"] and got["state"] == want["state"] == [1, want["iters"]]
    assert util.rel_err(got["pressure"], want["pressure"]) <= cpu.TOL
    assert rg <= rw + 1e-5 * float(np.abs(S["rhs"]).max())


def test_world_y_cut_preconditioner_on_hip(hip, oracle):
    want, got = cpu.world_run(oracle, "32x24x40", 2, blocking=(8, 0)), cpu.world_run(hip, "32x24x40", 2, blocking=(8, 0))
    assert got["iters"] == want["iters"] and got["state"] == want["state"]
    assert util.rel_err(got["pressure"], want["pressure"]) <= cpu.TOL


@pytest.mark.parametrize("stop", ["converged", "diverged"])
@pytest.mark.parametrize("extra", [1, 5])
@pytest.mark.parametrize("nranks", [1, 3], ids=lambda n: "nranks-%d" % n)
@pytest.mark.parametrize("name", list(cpu.WORLD_SYSTEMS))
def test_iterations_queued_past_the_stop_are_noops(hip, name, nranks, extra, stop):
    cpu.check_extra_is_noop(hip, name, nranks, extra, 3 if stop == "diverged" else None)
