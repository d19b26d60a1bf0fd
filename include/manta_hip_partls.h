/*
 * manta_hip_partls.h -- C ABI extension of `libmanta_hip.so`: the two smooth particle level sets of source/plugin/flip.cpp,
 * averagedParticleLevelset (Zhu & Bridson, :365-499) and improvedParticleLevelset (Solenthaler's Jacobian-corrected variant,
 * :501-581): the weighted gather over the particles of the (2r+1)^3 cells around every cell, the eigenvalue correction, the
 * smoothing passes and the final setBound(0.5, 0).
 *
 * It sits beside include/manta_hip.h and leaves that header (and MF_ABI_VERSION) as it is: a library either implements the whole
 * extension, reporting MF_PARTLS_ABI_VERSION through mf_partls_abi_version(), or none of it.  Conventions (error plumbing, borrowed
 * device pointers, SoA Vec3 grids, particle vectors with component stride `pstride`, idx = i + sx*(j + sy*k), streams) are those of
 * include/manta_hip.h.  The entry does not know the z-slab window (mf_set_slab_window): grids are whole domains.  It is
 * asynchronous on the stream and reads nothing back.
 */
#ifndef MANTA_HIP_PARTLS_H
#define MANTA_HIP_PARTLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_partls_levelset */
#define MF_PARTLS_ABI_VERSION 1
int mf_partls_abi_version(void);

/* averagedParticleLevelset (improved = 0) / improvedParticleLevelset (improved = 1), flip.cpp:365-581, bit for bit up to the
 * rounding of the device's fp64 pow/acos/cos/sin in the eigenvalue routine of the improved form (util/matrixbase.h:184-221).
 *   pos, indexSys, n_indexed, index : the particle positions and the result of mf_grid_particle_index
 *   phi        : [n], overwritten everywhere
 *   pAcc, rAcc : scratch, [3][n] and [n]; read and written only when improved (may be NULL otherwise)
 *   tmp        : scratch, [n]; may be NULL when smoothen <= 0 and smoothenNeg <= 0
 *   ptype      : nullable; particles with ptype & exclude are skipped
 * Per cell the weights w = max(0, 1 - |x - p|^2 / (4 radius^2)) are summed in the reference's order (zj, yj, xj, slot). */
int mf_partls_levelset(int sx, int sy, int sz, int64_t np, int64_t pstride, const float* pos, const int32_t* indexSys,
                       int64_t n_indexed, const int32_t* index, float* phi, float radiusFactor, int smoothen, int smoothenNeg,
                       int improved, float t_low, float t_high, const int32_t* ptype, int exclude, float* pAcc, float* rAcc,
                       float* tmp, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_PARTLS_H */
