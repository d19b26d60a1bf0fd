"""GPU: the users of the library's growable per-device scratch blocks (arena_reserve, csrc/runtime.hip) -- gridParticleIndex
(the scan / sort workspace of surface.hip), markFluidAndBoundaryCells + mapMassToGrid (idp.hip) and adjustNumber with a compress
(resample.hip, which also keeps its compress plan inside the block) -- through one sequence of sizes in one process, so that a block
is first allocated, regrown to a request of more than twice its size, reused by a smaller call, and regrown by doubling.  Every call
is compared, bit for bit, with what the plugins' own GPU tests compare with: tests/partls_model.py (particle_index),
tests/idp_model.py and tests/nbflip_model.py, through the helpers of tests/test_gpu_idp.py and tests/test_gpu_nbflip.py.
The ordered particle->grid transfer (p2g_ordered.hip) and the padded copy of mf_cg_solve (pressure.hip) go through the same branches
with sequences of their own, through the C ABI: the transfer bit for bit against the oracle's serial scatter (tests/p2g_cases.py),
the solve at the bars of tests/test_gpu_pcg_routes.py.

The blocks live as long as the process.  Inside the whole suite earlier tests may have left them large, which reduces this file to
the reuse branch; run on its own (`pytest tests/test_gpu_scratch_regrow.py`) it takes every branch."""
import numpy as np
import pytest

import cases
import idp_model as IM
import nbflip_model as NM
import p2g_cases as C
import partls_model as PM
import test_gpu_idp as TI
import test_gpu_nbflip as TN
import test_gpu_pcg_routes as TR
import util

pytestmark = pytest.mark.gpu

ADJUST_CALL = dict(minParticles=3, maxParticles=5, narrowBand=2.5)

# (dims, the branch of arena_reserve a fresh process takes, seed, options of nbflip_model.adjust_inputs, options of
# idp_model.mass_inputs).  Particles: about 190 / 150 in the small grid, 16 500 / 14 600 in step 2, 18 900 / 18 000 in step 4; the
# requests grow with the cells and with the particles, and both are larger in step 4 than in step 2, by less than a factor of two
SMALL = (dict(max_per_cell=2, dense_frac=0.1, outside=4), dict(per_axis=3, thin=0.15))
STEPS = [
    ((8, 6, 5), "first allocation", 1) + SMALL,
    ((24, 20, 18), "need > 2 cap", 2, dict(max_per_cell=16, dense_frac=0.2), dict(fill=0.47)),
    ((8, 6, 5), "a smaller call inside the larger block", 1) + SMALL,
    ((26, 20, 18), "cap < need <= 2 cap: doubling", 4, dict(max_per_cell=17, dense_frac=0.21), dict(fill=0.51)),
    ((20, 16, 1), "2-D", 5, {}, {}),
]


def _grid_particle_index(m, dims, pos, pflag):
    s = TI._solver(m, dims)
    pp, _ = TI._parts(m, s, pos, pflag)
    flags, gpi, pindex = s.create(m.FlagGrid), s.create(m.IntGrid), s.create(m.ParticleIndexSystem)
    m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
    start, _, isys = PM.particle_index(dims, pos, pflag)
    assert pindex.np == len(isys)
    assert np.array_equal(gpi.to_numpy().ravel(), start)
    assert np.array_equal(pindex.data[:pindex.np].cpu().numpy(), isys)
    return len(isys)


def _density_projection(m, dims, I):
    out, stats = TI.run_case(m, "mark", dims, I, dict(ptype=False))
    fl, dX, info = IM.mark_fluid_and_boundary(I["pos"], I["pflag"], I["flags"], I["phiObs"], None, 0)
    assert stats["boundary_particles"] == info["boundary"] and stats["pushing"] == info["pushing"]
    for k, v in dict(flags=fl, deltaX=dX).items():
        util.assert_bitexact(out[k], v, "mark " + k)
    out, stats = TI.run_case(m, "mass", dims, I, dict(noClamp=False))
    fl, d, dX, st = IM.map_mass_to_grid(I["flags"], I["pos"], I["pflag"], I["phiObs"], I["dt"], I["mass"], False)
    assert stats["flipped"] == st["flipped"] and stats["boundary_particles"] == st["boundary"]
    assert stats["candidates"] == st["candidates"] and stats["rounds"] == st["rounds"]
    for k, v in dict(flags=fl, density=d, deltaX=dX).items():
        util.assert_bitexact(out[k], v, "mass " + k)


def _adjust_number(m, dims, I):
    I["parts"].allow_compress = True
    want = TN._model_call(I, (0, 0), True, ADJUST_CALL)
    got = TN._run_device(m, I, [((0, 0), ADJUST_CALL)], dims)[0]
    TN._compare_state(got, want, "adjustNumber")
    assert got["stats"]["compresses"] >= 1 and got["stats"]["rounds"] == want.rounds
    return got["stats"]


def test_the_scratch_users_through_first_allocation_regrow_reuse_and_doubling(hip_backend):
    import manta as m
    for step, (dims, branch, seed, adjust_opt, mass_opt) in enumerate(STEPS, 1):
        A = NM.adjust_inputs(dims, 200 + seed, **adjust_opt)
        I = IM.mass_inputs(dims, 300 + seed, **mass_opt)
        indexed = _grid_particle_index(m, dims, A["parts"].pos, A["parts"].flag)
        _density_projection(m, dims, I)
        stats = _adjust_number(m, dims, A)
        print("step %d, %dx%dx%d (%s): %d particles indexed of %d, %d in the density projection, adjustNumber %s"
              % (step, *dims, branch, indexed, A["parts"].size(), len(I["pflag"]), stats))


# (input of p2g_cases, first m particles or None for all, branch).  The request of a call in bytes, with al(b) = b rounded up to 256
# and the plane stride cp = np + np // 8 + 1024 (p2g_ordered.hip, scratch_bytes):
#   4 al(4 np) + al(72 cp) + 2 al(4 (n + 1)) + al(4 n) + al(4 ((n + 1) // 4096 + 2)) + 256
# step 1: 88 832 (cp 1 031); step 2: 6 730 752 (68 140 particles, cp 77 681); step 3: 113 408 (cp 1 313); step 4: 10 202 624
# (cp 113 524), between once and twice step 2's -- d3 whole would ask for 16 483 328, more than twice; step 5: 4 229 376
P2G_STEPS = [
    ("patterns", 7, "first allocation"),
    ("hits", None, "need > 2 cap"),
    ("patterns", 257, "a smaller call inside the larger block, at another stride than step 1"),
    ("d3", 100000, "cap < need <= 2 cap: doubling"),
    ("d2", None, "2-D"),
]


def _p2g_request(np_, n):
    al = lambda b: (b + 255) & ~255
    cp = np_ + np_ // 8 + 1024
    return 4 * al(4 * np_) + al(72 * cp) + 2 * al(4 * (n + 1)) + al(4 * n) + al(4 * ((n + 1) // 4096 + 2)) + 256


def test_ordered_p2g_through_first_allocation_regrow_reuse_and_doubling(hip):
    """mf_map_parts_to_mac and mf_map_parts_to_grid (ncomp 1 and 3) with deterministic = 1: the ordered mode is the reference's serial
    scatter, so every output equals the oracle's bit for bit, whatever block and plane stride the call was cut"""
    req = []
    for step, (name, m, branch) in enumerate(P2G_STEPS, 1):
        inp, o = C.get(name), C.oracle_outputs(name, m)
        sx, sy, sz = inp.dims
        req.append(_p2g_request(inp.np if m is None else m, sx * sy * sz))
        print("step %d, %s[:%s] (%s): request %d bytes" % (step, name, m, branch, req[-1]))
        vel, velOld, w = C.run_mac(hip, inp, m, deterministic=1)
        util.assert_bitexact(w, o["weight"], "step %d: stomped weight" % step)
        util.assert_bitexact(vel, o["vel"], "step %d: finished vel" % step)
        util.assert_bitexact(velOld, o["velOld"], "step %d: velOld" % step)
        for ncomp in (1, 3):
            tgt, w = C.run_cell(hip, inp, ncomp, m, deterministic=1)
            util.assert_bitexact(w, o["wtmp%d" % ncomp], "step %d: weight sums, ncomp %d" % (step, ncomp))
            util.assert_bitexact(tgt, o["target%d" % ncomp], "step %d: target, ncomp %d" % (step, ncomp))
    assert req[1] > 2 * req[0] and req[2] < req[1] and req[1] < req[3] <= 2 * req[1] and req[4] < req[3], req


# (shape of cases.PCG_ROUTES with a padded internal copy, padded cells px * sy * sz, branch).  The request is 11 slices of
# al(4 * cells) bytes: 95 744, 422 400, 95 744, 684 288 (the block doubles to 844 800), 506 880
PAD_STEPS = [
    ((17, 9, 10), 2160, "first allocation"),
    ((33, 20, 12), 9600, "need > 2 cap"),
    ((17, 9, 10), 2160, "reuse"),
    ((65, 24, 9), 15552, "cap < need <= 2 cap: doubling"),
    ((63, 18, 10), 11520, "reuse, pad 1"),
]


def test_padded_cg_solve_through_first_allocation_regrow_reuse_and_doubling(hip, oracle):
    """mf_cg_solve with the MIC preconditioner on shapes whose rows are padded to a multiple of 8, on the inputs and at the bars of
    test_gpu_pcg_routes.test_cg_route"""
    routes = dict(cases.PCG_ROUTES)
    req = []
    for step, (dims, cells, branch) in enumerate(PAD_STEPS, 1):
        assert "padded" in routes[dims] and ((dims[0] + 7) & ~7) * dims[1] * dims[2] == cells
        req.append(11 * ((4 * cells + 255) & ~255))
        flags, A, _ = cases.system_inputs(dims, 5)
        rhs = cases.cg_rhs(dims, flags, 5)
        for acc, iters in ((1e-9, 4), (1e-3, 400)):
            got, want, _ = TR._check_solve(hip, oracle, dims, flags, A, rhs, 2, acc, iters, what="step %d, %s (%s)" % (step, dims, branch))
            print("step %d, %dx%dx%d (%s), request %d bytes, accuracy %g: %s" % (step, *dims, branch, req[-1], acc, got and got[1]))
    assert req[1] > 2 * req[0] and req[1] < req[3] <= 2 * req[1] and req[4] <= 2 * req[1], req
