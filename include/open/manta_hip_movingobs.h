/*
 * manta_hip_movingobs.h -- C ABI extension of `libmanta_hip.so`: a solid that moves through the fluid, and the obstacle coupling that
 * scenes/zflip.py and flip06_obstacle.py run every step between advection and the pressure solve:
 *   MovingObstacle            source/movingobs.cpp (moveLinear :55-93, projectOutside :39-53)
 *   particle projection       KnProjectParticles, source/particle.h:551-578
 *   wall conditions           kn_set_wall_bcs2, source/plugin/extforces.cpp:337-373
 *   MAC boundary bands        knSetBoundaryMAC, knSetBoundaryMACNorm, kn_set_bound_MAC2, source/grid.cpp:672-715
 *   flag helpers              mark_surface, clear_obstacle, source/grid.cpp:930-985 (get_ne_directions :113-131, is_boundary grid.h:447-458)
 *   norm clamp                knGridClampNorm, source/grid.cpp:306-319
 *   obstacle level set glue   knUnprojectNormalComp inside extrapolateMACSimple, source/fastmarch.cpp:303-375; knResetPhiInObs,
 *                             source/plugin/advection.cpp:397-402; GradientOp, source/commonkernels.h:67-72
 *
 * It lives under include/open/ with the other open extensions and follows their rules: include/manta_hip.h and MF_ABI_VERSION stay as
 * they are, a library either implements the whole extension, reporting MF_MOVINGOBS_ABI_VERSION through mf_movingobs_abi_version(), or
 * none of it.  Conventions (error plumbing, borrowed device pointers, SoA Vec3 grids, idx = i + sx*(j + sy*k), a stream as the last
 * argument) are those of include/open/manta_hip_fields.h.  The entries do not know the z-slab window: grids are whole domains.
 * "Interior" is KERNEL(bnd = 1): 1 <= i < sx-1, 1 <= j < sy-1 and, where sz > 1, 1 <= k < sz-1.  Every entry is one launch and
 * asynchronous unless it says otherwise; the one synchronising read-back is in mf_movingobs_project_count.  Scratch arrays are the
 * caller's.  Flag bits are those of include/manta_hip.h (MF_FLUID 1, MF_OBSTACLE 2, MF_EMPTY 4); TypeSurface is 128.  DESIGN.md
 * section 24 has the fp32 / fp64 map and the 2-D stride trap.
 */
#ifndef MANTA_HIP_MOVINGOBS_H
#define MANTA_HIP_MOVINGOBS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_movingobs_set_wall_bcs2, mf_movingobs_set_bound_mac, mf_movingobs_mark_surface, mf_movingobs_clear_obstacle,
 *      mf_movingobs_clamp_norm, mf_movingobs_reset_phi_in_obs, mf_movingobs_extrapolate_mac_simple, mf_movingobs_move,
 *      mf_movingobs_obstacle_sign, mf_movingobs_gradient, mf_movingobs_project_scratch, mf_movingobs_project_count,
 *      mf_movingobs_project_apply */
#define MF_MOVINGOBS_ABI_VERSION 1
int mf_movingobs_abi_version(void);

/* the most shapes one mf_movingobs_move call takes: they travel as kernel arguments */
#define MF_MOVINGOBS_MAX_SHAPES 16

/* kn_set_wall_bcs2, every cell: where i > 0 and one of the cells (i-1, i) is fluid and one of them is an obstacle, vel.x = obvel.x; the
 * same along y; along z on a 3-D grid, while on a 2-D grid vel.z = 0 in EVERY cell.  vel may not alias obvel. */
int mf_movingobs_set_wall_bcs2(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* obvel, void* stream);

/* the three band rules of a MAC grid, each with its own band per component (w = boundaryWidth; the z conditions hold on 3-D grids only):
 *   rule 0  knSetBoundaryMAC      x: i <= w || i >= sx-w   || j <= w-1 || j >= sy-1-w || k <= w-1 || k >= sz-1-w ; y, z by rotation
 *   rule 1  knSetBoundaryMACNorm  x: i <= w || i >= sx-w ; y: j <= w || j >= sy-w ; z: k <= w || k >= sz-w (never on a 2-D grid)
 *   rule 2  kn_set_bound_MAC2     x: i <= w+1 || i >= sx-1-w || j <= w || j >= sy-1-w || k <= w || k >= sz-1-w ; y, z by rotation */
int mf_movingobs_set_bound_mac(int sx, int sy, int sz, float* vel, float valueX, float valueY, float valueZ, int w, int rule, void* stream);

/* FlagGrid::mark_surface: TypeSurface is cleared in every cell, then set in every fluid cell that has, among its 26 (2-D: 8)
 * neighbours, one outside the grid, or one that is not on the outermost layer of the domain and is not fluid.  In place: a thread
 * changes the TypeSurface bit of its own cell only and reads the TypeFluid bit of the others, with relaxed atomic accesses. */
int mf_movingobs_mark_surface(int sx, int sy, int sz, int32_t* flags, void* stream);

/* FlagGrid::clear_obstacle: every obstacle cell becomes TypeEmpty (the whole word); with include_boundary == 0 the cells of the
 * outermost layer of the domain keep their flags */
int mf_movingobs_clear_obstacle(int sx, int sy, int sz, int32_t* flags, int include_boundary, void* stream);

/* knGridClampNorm on n elements of ncomp (1 or 3) planes: n_ = sqrtf(x*x (+ y*y + z*z)) in fp32, left to right; where n_ > val every
 * component is multiplied by the one fp32 quotient val / n_ */
int mf_movingobs_clamp_norm(int64_t n, int ncomp, float* data, float val, void* stream);

/* knResetPhiInObs: sdf = 0.1 (the double literal, rounded) in obstacle cells with sdf < 0 */
int mf_movingobs_reset_phi_in_obs(int64_t n, const int32_t* flags, float* sdf, void* stream);

/* extrapolateMACSimple with phiObs: the component passes of mf_extrapolate_mac_simple (the same device code), then
 * knUnprojectNormalComp on the interior -- where -maxDist <= phiObs <= 0 (maxDist = float(distance)) and dot(n, v) < 0 for the central
 * difference n of phiObs (centre clamped to [1, size-2]; no z difference in 2-D) and v = vel of the cell, vel -= n_ * dot(n_, v) with
 * n_ = normalize(n), all fp32 -- then the into-boundary copy.  tmp: n int32, velTmp: 3n floats.  2 + dim * (1 + distance) launches and
 * one device copy. */
int mf_movingobs_extrapolate_mac_simple(int sx, int sy, int sz, const int32_t* flags, float* vel, int distance, int intoObs,
                                        const float* phiObs, int32_t* tmp, float* velTmp, void* stream);

/* MovingObstacle::moveLinear after the host has eased alpha, moved the shapes and computed v; TWO launches whatever nshapes is.
 * The flag pass: a cell that carries `id` becomes emptyType, then a cell whose centre lies in any of the shapes becomes
 * MF_OBSTACLE | id.  The velocity pass over the interior reads the NEW flags: vel.x = vx where the cell or (i-1) carries id, vel.y = vy
 * where the cell or (j-1) does, vel.z = vz where the cell or (k-1) does -- on a 2-D grid the reference's z stride is 0, so "(k-1)" is
 * the cell itself and vel.z = vz wherever the cell carries id.  kinds_host: nshapes ints, params_host: nshapes * 12 floats, the
 * records of mf_shape_apply_to_grid, read on the host at call time; 0 <= nshapes <= MF_MOVINGOBS_MAX_SHAPES. */
int mf_movingobs_move(int sx, int sy, int sz, int32_t* flags, float* vel, int id, int emptyType, int nshapes, const int32_t* kinds_host,
                      const float* params_host, float vx, float vy, float vz, void* stream);

/* the start of MovingObstacle::projectOutside: phi = -0.5 in obstacle cells, 0.5 in the others */
int mf_movingobs_obstacle_sign(int64_t n, const int32_t* flags, float* phi, void* stream);

/* GradientOp on the interior: 0.5 * (central differences) per component, z = 0 on a 2-D grid; border cells of grad keep their values */
int mf_movingobs_gradient(int sx, int sy, int sz, const float* phi, float* grad, void* stream);

/* KnProjectParticles in three steps.  The reference's loop is serial because every active particle draws from one random stream: one
 * real first if its position is inside the grid (isInBounds(toVec3i(pos))), then three.  An inactive particle (MF_PDELETE) draws none.
 *   mf_movingobs_project_scratch  *bytes = the scratch mf_movingobs_project_count needs for np particles
 *   mf_movingobs_project_count    offsets[p] = the number of reals drawn before particle p, offsets[np] = their total (np + 1 int32), by
 *                                 one counting kernel and one exclusive scan; *total_host = offsets[np].  SYNCHRONISES the stream: the
 *                                 one read-back of the projection (8 bytes)
 *   mf_movingobs_project_apply    reals: offsets[np] floats on the device, drawn by the host from the persistent stream.  Inside the
 *                                 grid: n = interpol(grad, pos), dist = normalize(n), pos += n * (-dist + 0.1 * (1 + r0)) with 1 + r0 in
 *                                 fp32 and the factor in fp64, each product rounded once.  Then pos = clamp(pos, 1 + jit, size - 1 - jit)
 *                                 with jit = float(0.1 * r) per component, in fp32. */
int mf_movingobs_project_scratch(int64_t np, int64_t* bytes);
int mf_movingobs_project_count(int sx, int sy, int sz, int64_t np, int64_t pstride, const float* pos, const int32_t* pflag, int32_t* offsets,
                               void* tmp, int64_t tmp_bytes, int64_t* total_host, void* stream);
int mf_movingobs_project_apply(int sx, int sy, int sz, int64_t np, int64_t pstride, float* pos, const int32_t* pflag, const float* grad,
                               const int32_t* offsets, const float* reals, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_MOVINGOBS_H */
