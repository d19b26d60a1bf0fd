"""GPU: the three users of the library's growable per-device scratch blocks (arena_reserve, csrc/runtime.hip) -- gridParticleIndex
(the scan / sort workspace of surface.hip), markFluidAndBoundaryCells + mapMassToGrid (idp.hip) and adjustNumber with a compress
(resample.hip, which also keeps its compress plan inside the block) -- through one sequence of sizes in one process, so that a block
is first allocated, regrown to a request of more than twice its size, reused by a smaller call, and regrown by doubling.  Every call
is compared, bit for bit, with what the plugins' own GPU tests compare with: tests/partls_model.py (particle_index),
tests/idp_model.py and tests/nbflip_model.py, through the helpers of tests/test_gpu_idp.py and tests/test_gpu_nbflip.py.

The blocks live as long as the process.  Inside the whole suite earlier tests may have left them large, which reduces this file to
the reuse branch; run on its own (`pytest tests/test_gpu_scratch_regrow.py`) it takes every branch."""
import numpy as np
import pytest

import idp_model as IM
import nbflip_model as NM
import partls_model as PM
import test_gpu_idp as TI
import test_gpu_nbflip as TN
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
