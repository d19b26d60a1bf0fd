/*
 * manta_hip_gridops.h -- C ABI extension of `libmanta_hip.so`: the grid operations and small grid plugins of the reference that no other
 * extension covers:
 *   axis permutation          knPermuteAxes, Grid::permuteAxes / permuteAxesCopyToGrid, source/grid.cpp:251-256, 322-339
 *   L1 / L2 norms             loop_calcL1Grid / loop_calcL2Grid, source/grid.cpp:387-418
 *   join                      knJoinVec / knJoinInt / knJoinReal, source/grid.cpp:258-268, 340-348
 *   force fields              KnApplyForceField, KnAddForceIfLower, source/plugin/extforces.cpp:24-43, 376-407, 430-436
 *   Vec3 extrapolation        extrapolateVec3Simple, source/fastmarch.cpp:434-468, 525-557
 *   emission, obstacle reset  KnApplyEmission, KnResetInObstacle, source/plugin/initplugins.cpp:110-128, 154-183
 *   layout converters         copyMACData, copyRealToVec3, copyVec3ToReal, resampleMacToVec3, swapComponents, getGridAvg,
 *                             source/grid.cpp:496-505, 516-536, 564-571, 717-739, 1013-1033; debugIntToReal, source/plugin/flip.cpp:266-269
 *   simple noise              knApplySimpleNoiseReal / knApplySimpleNoiseVec3, source/plugin/waveletturbulence.cpp:85-116
 *   legacy whitewater         the single-potential plugins, source/plugin/secondaryparticles.cpp:549-706
 *
 * It lives under include/open/ with the other open extensions and follows their rules: include/manta_hip.h and MF_ABI_VERSION stay as
 * they are, a library either implements the whole extension, reporting MF_GRIDOPS_ABI_VERSION through mf_gridops_abi_version(), or
 * none of it.  Conventions (error plumbing, borrowed device pointers, SoA Vec3 grids, idx = i + sx*(j + sy*k), a stream as the last
 * argument) are those of include/open/manta_hip_fields.h.  The entries do not know the z-slab window: grids are whole domains.
 * "Interior" is KERNEL(bnd = 1): 1 <= i < sx-1, 1 <= j < sy-1 and, where sz > 1, 1 <= k < sz-1.  Every entry is asynchronous unless it
 * says otherwise; the entries with a *_host result synchronise the stream for that one read-back.  Scratch arrays are the caller's.
 * Flag bits are those of include/manta_hip.h (MF_FLUID 1, MF_OBSTACLE 2, MF_EMPTY 4); TypeInflow is 8 and TypeOutflow 16.  DESIGN.md
 * section 25 has the fp32 / fp64 map, the tile's bank derivation and the bound of the fp64 sums.
 */
#ifndef MANTA_HIP_GRIDOPS_H
#define MANTA_HIP_GRIDOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_gridops_permute, mf_gridops_norm, mf_gridops_join, mf_gridops_force_field, mf_gridops_add_force_if_lower,
 *      mf_gridops_extrapolate_vec3_simple, mf_gridops_apply_emission, mf_gridops_reset_in_obstacle, mf_gridops_copy_mac_data,
 *      mf_gridops_copy_planes, mf_gridops_resample_mac_to_vec3, mf_gridops_swap_components, mf_gridops_grid_avg,
 *      mf_gridops_simple_noise, mf_gridops_legacy_potential, mf_gridops_neighbor_ratio, mf_gridops_surface_normals,
 *      mf_gridops_int_to_real */
#define MF_GRIDOPS_ABI_VERSION 1
int mf_gridops_abi_version(void);

/* the side of the square LDS tile of the transposing permutations, in 4-byte words, and its row pitch (one word of padding) */
#define MF_GRIDOPS_TILE 32
#define MF_GRIDOPS_TILE_PITCH 33

/* knPermuteAxes on ncomp planes of 4-byte words (int, Real, or the three planes of a Vec3 grid): target(s[axis0], s[axis1], s[axis2]) =
 * self(s[0], s[1], s[2]) for every source cell s.  The source is sx x sy x sz; the target MUST be S[axis0] x S[axis1] x S[axis2] with
 * S = (sx, sy, sz) -- the caller has checked that, the entry derives the target's strides from it.  (axis0, axis1, axis2) is a
 * permutation of (0, 1, 2); anything else is refused.  axis0 == 0 keeps x fastest: a row copy.  The four permutations that move x go
 * through a MF_GRIDOPS_TILE x MF_GRIDOPS_TILE tile in LDS so that the global read and the global write both run along x.  dst may not
 * overlap src.  One launch. */
int mf_gridops_permute(int sx, int sy, int sz, int axis0, int axis1, int axis2, int ncomp, const void* src, void* dst, void* stream);

/* Grid::getL1 (l2 == 0) / getL2 (l2 == 1) over bnd <= i < sx-bnd, bnd <= j < sy-bnd and, where sz > 1, bnd <= k < sz-bnd.  kind 0 Real:
 * |v| or the fp32 product v*v; kind 1 int: float(abs(v)) or float(v*v) with the product in 32-bit integers; kind 2 Vec3 (SoA): norm()
 * with its two epsilon branches (vectorbase.h:385-389) or the fp32 x*x + y*y + z*z.  The terms are summed in fp64 (per thread, wavefront
 * shuffle, per block, one finishing block: a fixed order); *result_host = (float)sum or (float)sqrt(sum).  An empty range gives 0.
 * SYNCHRONISES the stream: 8 bytes are read back. */
int mf_gridops_norm(int kind, int l2, int sx, int sy, int sz, int bnd, const void* a, float* result_host, void* stream);

/* Grid::join on n cells.  kind 0 Real, kind 1 int: a = keepMax ? max(a, b) : min(a, b) (std::max / std::min: a where the two compare
 * equal or unordered).  kind 2 Vec3 (SoA): every component of a becomes max / min of the two fp32 normSquares. */
int mf_gridops_join(int kind, int64_t n, void* a, const void* b, int keepMax, void* stream);

/* KnApplyForceField on the interior: nothing in a cell that is neither fluid nor empty, nor where region (nullable) > 0.  The force at a
 * face is force(cell) with isMAC, else 0.5 * (force(lower neighbour) + force(cell)) with the sum in fp32; the z component on 3-D grids
 * only.  A component is written where the lower neighbour is fluid, or the cell is fluid and the lower neighbour empty: vel += force
 * with additive, else vel = force. */
int mf_gridops_force_field(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* force, const float* region, int additive,
                           int isMAC, void* stream);

/* KnAddForceIfLower (setInitialVelocity) on the interior, on the same faces: f = 0.5 * (force(lower) + force(cell));
 * vel = f > 0 ? min(vel + f, max(vel, f)) : max(vel + f, min(vel, f)) */
int mf_gridops_add_force_if_lower(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* force, void* stream);

/* extrapolateVec3Simple: tmp = 1 in interior cells with phi < 0 (inside: phi > 0), 2 in the other interior cells with such a 6- (2-D: 4-)
 * neighbour, else 0; for d = 2 .. distance a pass over the interior cells with tmp == 0 that have neighbours with tmp == d: vel = (sum of
 * their vel, in the order +x -x +y -y +z -z) / float(count) + 0 per component, tmp = d + 1; at the end vel = 0 in every interior cell with
 * tmp == 0.  tmp: n int32, overwritten.  1 + max(distance - 1, 0) + 1 launches. */
int mf_gridops_extrapolate_vec3_simple(int sx, int sy, int sz, float* vel, const float* phi, int distance, int inside, int32_t* tmp,
                                       void* stream);

/* KnApplyEmission, every cell: skipped only where BOTH hold -- type != 0 and the cell is neither (type & 8 and inflow) nor (type & 16 and
 * outflow), AND emissionTexture is given and 0 there; else target = source (isAbsolute) or target += source */
int mf_gridops_apply_emission(int64_t n, const int32_t* flags, float* target, const float* source, const float* emissionTexture,
                              int isAbsolute, int type, void* stream);

/* KnResetInObstacle, every obstacle cell: the three components of vel and each given grid = resetValue.  density, heat, fuel, red are
 * nullable; flame is written only with fuel, green and blue only with red (they must be given then). */
int mf_gridops_reset_in_obstacle(int64_t n, const int32_t* flags, float* vel, float* density, float* heat, float* fuel, float* flame,
                                 float* red, float* green, float* blue, float resetValue, void* stream);

/* copyMACData: target = source (three components) where flags & flag, over the range of mf_gridops_norm for bnd */
int mf_gridops_copy_mac_data(int sx, int sy, int sz, const float* source, float* target, const int32_t* flags, int flag, int bnd,
                             void* stream);

/* copyRealToVec3 / copyVec3ToReal in SoA storage: dst0 = src0, dst1 = src1, dst2 = src2 on n words each, one launch */
int mf_gridops_copy_planes(int64_t n, const float* src0, const float* src1, const float* src2, float* dst0, float* dst1, float* dst2,
                           void* stream);

/* knResampleMacToVec3 on the interior: target = source.getCentered(i, j, k) = 0.5 * (v(cell) + v(upper neighbour)) per component with the
 * sum in fp32, z = 0 on a 2-D grid; the border of target keeps its values.  target may not alias source. */
int mf_gridops_resample_mac_to_vec3(int sx, int sy, int sz, const float* source, float* target, void* stream);

/* swapComponents: (x, y, z) = (v[c1], v[c2], v[c3]) of the old value v in every cell; 0 <= c1, c2, c3 <= 2, repeats allowed */
int mf_gridops_swap_components(int64_t n, float* vel, int c1, int c2, int c3, void* stream);

/* getGridAvg: the fp64 sum (the order of mf_gridops_norm) of source over every cell, or over the fluid cells of flags (nullable), times
 * 1. / count in fp64, rounded to fp32; -1 where the count is 0.  SYNCHRONISES the stream: 16 bytes are read back. */
int mf_gridops_grid_avg(int64_t n, const float* source, const int32_t* flags, float* result_host, void* stream);

/* applySimpleNoiseReal (vec == 0) / applySimpleNoiseVec3 (vec != 0): on fluid cells target += noise.evaluate(c) * scale * factor, or
 * noise.evaluateCurl(c) * scale * factor per component, with c = (i + 0.5, j + 0.5, k + 0.5) and factor = weight(cell) or 1 where weight is
 * NULL; fp32 products left to right.  tile: the 3 x 128^3 wavelet tile, params: the 20 floats of mf_add_noise / mf_apply_noise_vec3
 * (read on the host at call time); the evaluators are theirs. */
int mf_gridops_simple_noise(int vec, int sx, int sy, int sz, const int32_t* flags, float* target, const float* tile, const float* params,
                            float scale, const float* weight, void* stream);

/* The legacy single-potential whitewater plugins (secondaryparticles.cpp:549-658), one launch: pot = 0, then in every cell with
 * flags & itype -- of the interior for which 0 and 1, of the whole grid for 2 --
 *   which 0  flipComputePotentialTrappedAir     sum over the neighbours within radius with flags & jtype of |vij| (1 - vij^ . xij^) (1 - |xij| / h)
 *   which 1  flipComputePotentialWaveCrest      sum over those with xij^ . ni < 0 of (1 - ni . nj) (1 - |xij| / h); 0 unless vi^ . ni >= 0.6
 *   which 2  flipComputePotentialKineticEnergy  62.5 |vi|^2 (radius, jtype and normal are not read)
 * clamped as (min(p, tauMax) - min(p, tauMin)) / (tauMax - tauMin); x = scaleFromManta * cell index, v = scaleFromManta * getCentered,
 * h = float(1.732 * radius), in 2-D float(1.414 * radius); neighbours x outer, y, z inner, z over k - radius .. k + radius in 2-D as well,
 * where the z stride is 0 and the plane is met again with another z in xj (the reference's arithmetic).  The reference reads outside
 * the grid unless every itype cell is radius cells from each side and no visited neighbour lies on the upper outermost layer; here a
 * neighbour whose words fall outside the array is skipped.  normal: 3n floats, needed by which 1.  0 <= radius <= 16. */
int mf_gridops_legacy_potential(int which, int sx, int sy, int sz, float* pot, const int32_t* flags, const float* vel, const float* normal,
                                int radius, float tauMin, float tauMax, float scaleFromManta, int itype, int jtype, void* stream);

/* flipUpdateNeighborRatio (:674-706): ratio = 0, then in the interior cells with flags & itype the number of neighbours within radius
 * with flags & itype over the number without flags & jtype (jtype means "skip" here), as float / float: NaN where there is none */
int mf_gridops_neighbor_ratio(int sx, int sy, int sz, const int32_t* flags, float* ratio, int radius, int itype, int jtype, void* stream);

/* flipComputeSurfaceNormals (:662-670): normal = GradientOp(phi) on the interior, then getNormalized(normal) in every cell, in place */
int mf_gridops_surface_normals(int sx, int sy, int sz, float* normal, const float* phi, void* stream);

/* debugIntToReal: dest = float(source) * factor */
int mf_gridops_int_to_real(int64_t n, const int32_t* source, float* dest, float factor, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_GRIDOPS_H */
