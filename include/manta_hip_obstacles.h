/*
 * manta_hip_obstacles.h -- C ABI extension of `libmanta_hip.so`: fill-fraction obstacle boundaries
 * (mantaflow's second-order obstacle boundaries: a levelset phiObs plus fill fractions on the MAC faces).
 *
 * It sits beside include/manta_hip.h and leaves that header (and MF_ABI_VERSION) as it is: a library either
 * implements the whole extension, reporting MF_OBSTACLES_ABI_VERSION through mf_obstacles_abi_version(), or none
 * of it.  Conventions (error plumbing, borrowed device pointers, SoA Vec3/MAC grids, idx = i + sx*(j + sy*k),
 * streams) are those of include/manta_hip.h.  Every entry cites the reference KERNEL() / PYTHON() it replaces and
 * reproduces it bit for bit.  None of them knows the z-slab window (mf_set_slab_window): grids are whole domains.
 */
#ifndef MANTA_HIP_OBSTACLES_H
#define MANTA_HIP_OBSTACLES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  updateFractions, setObstacleFlags, setWallBcs (fraction mode), setInflowBcs, addNoise */
#define MF_OBSTACLES_ABI_VERSION 1
int mf_obstacles_abi_version(void);

/* updateFractions -> fractions.setConst(0) + KnUpdateFractions (KERNEL(bnd=1)), plugin/initplugins.cpp:351-440.
 * Writes every face of `fractions` (MAC, SoA).  The result is the one of the reference's serial i, j, k sweep (one thread):
 * the "max" rules' writes into a +1 neighbour survive only where that neighbour lies outside the bnd=1 range.  The "max z"
 * rule tests j >= sz - boundaryWidth - 2 as the reference does.  3-D grids need sz >= 3. */
int mf_update_fractions(int sx, int sy, int sz, const int32_t* flags, const float* phiObs, float* fractions, int boundaryWidth,
                        float fracThreshold, void* stream);

/* setObstacleFlags -> KnUpdateFlagsObs (KERNEL(bnd=boundaryWidth)), plugin/initplugins.cpp:442-474: overwrites the flag word of
 * every cell of the range with Obstacle / Fluid|Inflow / Empty|Outflow / Empty.  fractions, phiOut, phiIn nullable;
 * boundaryWidth >= 0, and >= 1 when fractions are given (the reference reads past the grid otherwise). */
int mf_set_obstacle_flags(int sx, int sy, int sz, int32_t* flags, const float* phiObs, const float* fractions, const float* phiOut,
                          const float* phiIn, int boundaryWidth, void* stream);

/* setWallBcs(flags, vel, obvel, fractions, phiObs) -> KnSetWallBcsFrac + vel.swap(tmpvel), plugin/extforces.cpp:240-335, in place:
 * every new face value is computed from the original velocities.  obvel and boundaryWidth are unused by the reference and not
 * passed.  scratch: device memory of at least mf_set_wall_bcs_frac_scratch_words() 32-bit words (contents need no initialisation);
 * it holds the new face values and one bit per face that marks them. */
int mf_set_wall_bcs_frac(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* phiObs, uint32_t* scratch,
                         int64_t scratchWords, void* stream);
/* the scratch size mf_set_wall_bcs_frac needs for a grid of sx*sy*sz cells (host output) */
int mf_set_wall_bcs_frac_scratch_words(int sx, int sy, int sz, int64_t* words_host);

/* setInflowBcs -> KnSetInflow, plugin/extforces.cpp:163-182: sets the whole Vec3 (vx, vy, vz) of every cell on the chosen sides.
 * sides: bit 0 'x', 1 'X', 2 'y', 3 'Y', 4 'z', 5 'Z'.  A lower side sets planes 0 and 1, an upper side plane size-1.  The
 * caller rejects a bad direction character (after applying the characters before it, as the reference does). */
int mf_set_inflow_bcs(int sx, int sy, int sz, float* vel, int sides, float vx, float vy, float vz, void* stream);

/* addNoise -> KnAddNoise, plugin/initplugins.cpp:45-51: density += noise.evaluate(Vec3(i,j,k)) * scale on fluid cells where
 * sdf is absent or sdf <= 0.  sdf nullable; tile and params (host, 20 floats) as for mf_density_inflow (manta_hip.h). */
int mf_add_noise(int sx, int sy, int sz, const int32_t* flags, float* density, const float* sdf, const float* tile,
                 const float* params_host, float scale, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_OBSTACLES_H */
