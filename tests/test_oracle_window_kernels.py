"""The oracle's z-slab window code, entry point by entry point (tests/window_cases.py), on the CPU: every case on the planes
[lo, hi) under mf_set_slab_window(lo, gsz) against the same case on the undivided grid, bit for bit on the planes (particles) left
after trimming the case's reach at every cut.  The undivided oracle is what tests/test_oracle_vs_reference.py pins to the compiled
reference; tests/test_gpu_window_kernels.py then holds the HIP library to it.

Guards against an empty test: at least 4 planes or 200 particles per comparison; for a reach > 0 something differs in the planes
trimmed away (the cut is live); for a case that depends on absolute z the same call without a window goes wrong."""
import pytest

import window_cases as wc


@pytest.mark.parametrize("win", list(wc.WINDOWS))
@pytest.mark.parametrize("name,shape", wc.PARAMS, ids=["%s-%s" % p for p in wc.PARAMS])
def test_window(oracle, name, shape, win):
    wc.check_oracle(oracle, name, shape, win)


def test_table_covers_the_window_entry_points():
    """every entry point whose reach the case table states is in it"""
    names = " ".join(wc.BY_NAME)
    for ep in ("semi_lagrange_real", "semi_lagrange_vec3", "semi_lagrange_mac", "maccormack_clamp-", "maccormack_clamp_mac", "maccormack_correct_clamp-",
               "maccormack_correct_clamp_mac", "maccormack_correct-", "maccormack_correct_mac", "plugins.advectSemiLagrange", "apply_outflow_bc",
               "set_wall_bcs", "add_buoyancy", "apply_force", "mark_isolated_fluid_cell", "compute_energy", "extrapolate_mac_simple",
               "extrapolate_mac_from_weight", "extrapolate_ls_simple", "vorticity_confinement", "shape_levelset", "shape_apply_to_grid",
               "grid_set_bound", "density_inflow", "apply_noise_vec3", "interpolate_grid", "interpolate_mac_grid", "grid_particle_index",
               "union_particle_levelset", "map_mac_to_parts", "flip_velocity_update", "map_grid_to_parts", "apic_map_mac_to_parts",
               "map_parts_to_mac_accum", "apic_map_parts_to_mac", "map_parts_to_grid", "advect_in_grid", "mark_fluid_cells", "project_out_of_bnd",
               "push_out_of_obs", "set_part_type", "reset_outflow", "plugins.resetOutflow"):
        assert ep in names, ep
    for c in wc.CASES:
        assert c.why and 0 <= c.reach <= 4
