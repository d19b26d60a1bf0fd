/*
 * manta_hip_idp.h -- C ABI extension of `libmanta_hip.so`: implicit density projection (IDP-FLIP / IDP-APIC, Kugelstadt et al.),
 * the position solve of source/plugin/implicitdensityprojection.cpp: the marking of fluid cells with the push-out displacements
 * of particles inside obstacles, the density of the particle distribution, the displacement field of the second Poisson solve and
 * its gather to the particle positions.  resampeOverfullCells is not part of it (it draws from std::random_device).
 *
 * It sits beside include/manta_hip.h and leaves that header (and MF_ABI_VERSION) as it is: a library either implements the whole
 * extension, reporting MF_IDP_ABI_VERSION through mf_idp_abi_version(), or none of it.  Conventions (error plumbing, borrowed device
 * pointers, SoA Vec3/MAC grids and particle vectors with component stride `pstride`, idx = i + sx*(j + sy*k), streams) are those of
 * include/manta_hip.h.  Every entry cites the reference lines it replaces and reproduces them bit for bit.  None of them knows the
 * z-slab window (mf_set_slab_window): grids are whole domains.
 *
 * The two serial loops of the reference (the particle loop of the marking, the in-place flag sweep of knComputeDensity) run as their
 * order-free statements ("Implicit density projection").  Working arrays live in a per-device arena of the library that
 * grows geometrically and never shrinks.
 */
#ifndef MANTA_HIP_IDP_H
#define MANTA_HIP_IDP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  markFluidAndBoundaryCells, the weight sum and knComputeDensity of mapMassToGrid, computeDeltaX, mapMACToPartPositions */
#define MF_IDP_ABI_VERSION 1
int mf_idp_abi_version(void);

/* markFluidAndBoundaryCells, implicitdensityprojection.cpp:29-79: fluid cells become empty, deltaX is zeroed, every cell that holds
 * an active particle (not excluded by ptype & exclude; ptype nullable) becomes fluid, and a particle inside an obstacle cell with
 * phiObs <= 0 at its position proposes -(max(phi, -1) + 1e-2) * grad phiObs (central differences, eps = 1e-3) on the two faces per
 * axis of its cell; a face keeps the proposal of largest magnitude, among equal magnitudes that of the lowest particle index (the
 * serial loop's strict `>`).  In 2-D no z component is written.  Cells that carry the obstacle bit together with the empty or fluid
 * bit are marked and take no proposal.  result_host (2 x int64, valid on return: the call synchronises the stream once):
 *   [0] active particles inside obstacle cells   [1] those of them with phiObs <= 0 (the ones that propose) */
int mf_idp_mark(int sx, int sy, int sz, int32_t* flags, float* deltaX, const float* phiObs, int64_t np, int64_t pstride,
                const float* pos, const int32_t* pflag, const int32_t* ptype, int exclude, int64_t* result_host, void* stream);

/* the particle->grid transfer of mapMassRealHelper, :168 -> knMapLinear :83-90: density = the sum of the trilinear weights of the
 * active particles, summed per node in particle-index order (the ordered transfer of mf_map_parts_to_grid without its value grid's
 * clear and division).  psrc: one Real per particle (read, its sum is discarded). */
int mf_idp_map_weights(int sx, int sy, int sz, float* density, int64_t np, int64_t pstride, const float* pos, const int32_t* pflag,
                       const float* psrc, void* stream);

/* knComputeDensity, :100-154, as the single-thread sweep (k outer, j, i inner) computes it: density holds the weight sums on entry.
 * The particle-deficiency loop of a 3-D cell sees the final flag of the 13 neighbours swept before it and the entry flag of itself
 * and the 13 after it.  Fluid cells must not lie on the outermost layer of the grid.  result_host (4 x int64, one stream
 * synchronise): [0] cells whose flip depended on earlier flips (candidates; 0 in 2-D)  [1] cells flipped to empty
 *               [2] rounds the candidates took  [3] 0 */
int mf_idp_compute_density(int sx, int sy, int sz, float* density, int32_t* flags, const float* deltaX, float dt, float mass,
                           int noDensityClamping, int64_t* result_host, void* stream);

/* computeDeltaX, :184-205: Lambda = 0 in empty cells (one cell off the sides), then per non-obstacle cell and axis
 * deltaX = Lambda - Lambda(lower neighbour) where that neighbour is no obstacle; every other component keeps its value.  A
 * neighbour outside the grid (the reference reads before the row) counts as an obstacle. */
int mf_idp_compute_delta_x(int sx, int sy, int sz, const int32_t* flags, float* deltaX, float* Lambda, void* stream);

/* mapMACToPartPositions, :207-245: pos += deltaX.getInterpolated(pos) * dt, then per component the clamp to [1.001, size - 1.001]
 * (z in 2-D: [-10.001, 10.001]) */
int mf_idp_map_mac_to_positions(int sx, int sy, int sz, const float* deltaX, int64_t np, int64_t pstride, float* pos,
                                const int32_t* pflag, const int32_t* ptype, int exclude, float dt, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_IDP_H */
