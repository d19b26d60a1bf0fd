"""CPU: the numpy model of the turbulence model (tests/turbulence_model.py) against the reference fixture tests/golden/turbulence.npz
(how each array was produced: tools/record_turbulence.py), bit for bit, and -- from the model's branch counters -- that the fixture's
cases really enter every branch they exist for.  Arrays of more than turbulence_model.FULL_LIMIT elements are in the fixture as the
SHA-256 of their bytes: the model regenerates the array and its digest must be the recorded one.

The particle cases run in turbulence_model.PARTICLE_ORDER on one continuing state, as they were recorded: seed()'s random stream and
synthesize()'s clock and inflow offset are process-wide in the reference.  advectInGrid is not restated in numpy: the model takes the
package's existing entry from the CPU checker library (turbulence_model.oracle_advect)."""
import os

import numpy as np
import pytest

import turbulence_model as M

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "turbulence.npz"))


def check(key, a):
    msg = M.same_as_fixture(GOLDEN, key, a)
    assert msg is None, msg


@pytest.mark.parametrize("name", M.PRODUCTION_CASES)
def test_production(name):
    with_strain, without = M.run_production(name, True), M.run_production(name, False)
    for key, a in with_strain.items():
        check("production/%s/%s" % (name, key), a)
    for key, a in without.items():           # strain = None changes no other output (the recorder asserted it of the reference)
        check("production/%s/%s" % (name, key), a)
    border = ~M.interior_mask(M.shape_of(M.DIMS[name]))
    for key in ("prod", "nuT", "strain"):
        assert np.array_equal(with_strain[key][border], M.prefill(name, key)[border])


@pytest.mark.parametrize("name", M.SOURCES_CASES)
def test_sources_and_bcs(name):
    for key, a in M.run_sources(name).items():
        check("sources/%s/%s" % (name, key), a)
    for fill in (False, True):
        for key, a in M.run_bcs(name, fill).items():
            check("bcs/%s/%d/%s" % (name, fill, key), a)


@pytest.mark.parametrize("with_vel", (False, True))
@pytest.mark.parametrize("name", M.GRADDIFF_CASES)
def test_gradient_diffusion_twice(name, with_vel):
    for key, a in M.run_graddiff(name, with_vel).items():
        check("graddiff/%s/%d/%s" % (name, with_vel, key), a)


@pytest.mark.parametrize("name", M.DIAG_CASES)
def test_diagnostics(name):
    r = M.run_diagnostics(name)
    for key, a in r.items():
        check("diag/%s/%s" % (name, key), a)
    border = ~M.interior_mask(M.shape_of(M.DIMS[name]))
    assert np.array_equal(r["vort"][border], M.diag_prefill_vec(name)[border]) and not r["curl2"][border].any()


def test_grid_cases_enter_every_branch():
    cnt = {}
    for name in M.PRODUCTION_CASES:
        M.run_production(name, True, cnt)
        M.run_production(name, False, cnt)
    for key in ("k_low", "k_high", "nu_high", "nu_low", "eps_nonpositive", "eps_nan", "eps_positive", "strain_none", "strain_given"):
        assert cnt.get(key, 0) > 0, (key, cnt)
    cnt = {}
    for name in M.SOURCES_CASES:
        M.run_sources(name, cnt)
    for key in ("ke_nonpositive", "newEps_nonpositive", "k_low", "k_high", "nu_high", "nu_low"):
        assert cnt.get(key, 0) > 0, (key, cnt)
    I = M.ke_inputs("g7")
    assert ((I["flags"] & M.TypeObstacle) != 0).any() and ((I["flags"] & M.TypeObstacle) == 0).any()
    assert (M.graddiff_inputs("g33")["nuT"][~M.interior_mask(M.shape_of(M.DIMS["g33"]))] < 0).any()     # a negative zero in `res`


def test_fill_in_boundary_order_matters_only_where_no_interior_cell_reads():
    """the in-place sweep gives edge and corner cells of the centred grid a value that depends on its order; face cells do not"""
    vc = M.get_centered(M.rand_vel("g7", 2.0))
    serial = M.fill_in_boundary(vc)
    k, j, i = np.meshgrid(*[np.arange(n) for n in vc.shape[:3]], indexing="ij")
    cl = lambda a, n: np.clip(a, 1, n - 2)
    clamped = vc[cl(k, vc.shape[0]), cl(j, vc.shape[1]), cl(i, vc.shape[2])]      # every border cell from its nearest interior cell
    on_border = lambda a, n: (a == 0) | (a == n - 1)
    faces = on_border(k, vc.shape[0]).astype(int) + on_border(j, vc.shape[1]) + on_border(i, vc.shape[2]) <= 1
    assert np.array_equal(serial[faces], clamped[faces])
    assert not np.array_equal(serial[~faces], clamped[~faces])


@pytest.fixture(scope="module")
def particle_runs():
    from mantaflow_amd import _lib
    tile, params = M.noise_tile_and_params(M.PDIMS)
    _lib.reset()
    st, cnt, runs = M.State(), {}, {}
    for name in M.PARTICLE_ORDER:
        start = st.snapshot()
        runs[name] = (start,) + M.run_particle_case(name, st, tile, params, cnt)
    return runs, cnt, st.snapshot()


@pytest.mark.parametrize("name", M.PARTICLE_ORDER)
def test_particle_case(particle_runs, name):
    start, state, sizes, cursors = particle_runs[0][name]
    assert np.array_equal(start, GOLDEN["parts/%s/start" % name])
    assert np.array_equal(sizes, GOLDEN["parts/%s/sizes" % name])            # the reference's sizes after every call
    assert np.array_equal(cursors, GOLDEN["parts/%s/cursors" % name])
    for c in M.CHANNELS:
        check("parts/%s/%s" % (name, c), state[c])


def test_particle_cases_enter_every_branch(particle_runs):
    runs, cnt, end = particle_runs
    for key in M.PARTICLE_CONDITIONS:
        assert cnt.get(key, 0) > 0, (key, cnt)
    assert np.array_equal(end, GOLDEN["loop/start"])           # the recorded loop began where the cases ended
    seq = runs["seq"]
    assert list(seq[2][:3]) == [200, 300, 450]                   # three seeding calls on the continuing stream
    assert seq[3][0] - runs["n5000"][3][-1] > 3 * 200            # the sphere rejected attempts: more than three reals per particle
    assert list(runs["all"][2]) == [40, 0] and list(runs["none"][2]) == [40, 40] and list(runs["last"][2]) == [10, 10, 9]
    assert runs["n0"][2][-1] == 0 and runs["n1"][2][-1] == 1
    for n in (63, 64, 65, 1000, 5000):
        assert 0 < runs["n%d" % n][2][-1] < n                    # some deleted


def test_loop_record_is_what_the_issue_asks_for():
    per_step = GOLDEN["loop/per_step"]
    assert per_step.shape == (M.LOOP["steps"], 2) and (per_step > 0).all()
    assert GOLDEN["loop/obstacle_cells"][0] >= 16                # the 16 spheres of radius 1 still mark cells at res 40
    assert per_step[-1, 0] < 500 * M.LOOP["steps"]               # and particles are deleted in them
    assert per_step[0, 0] == 500                                 # the seeding box has volume
