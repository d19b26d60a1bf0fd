/*
 * manta_hip_resample.h -- C ABI extension of `libmanta_hip.so`: particle resampling for narrow-band FLIP
 * (adjustNumber with the particle system's delete / compress bookkeeping and the buffered insertion, combineGridVel)
 * and the two grid operations its scenes call (Grid::setBoundNeumann, LevelsetGrid::initFromFlags).
 *
 * It sits beside include/manta_hip.h and leaves that header (and MF_ABI_VERSION) as it is: a library either
 * implements the whole extension, reporting MF_RESAMPLE_ABI_VERSION through mf_resample_abi_version(), or none
 * of it.  Conventions (error plumbing, borrowed device pointers, SoA Vec3/MAC grids and particle vectors with component
 * stride `pstride`, idx = i + sx*(j + sy*k), streams) are those of include/manta_hip.h.  Every entry cites the reference
 * lines it replaces and reproduces them bit for bit.  None of them knows the z-slab window (mf_set_slab_window): grids
 * are whole domains.
 *
 * The serial particle loop of adjustNumber is replaced by its order-free statement ("Particle resampling"):
 * the caller runs mf_resample_round from i0 = 0 until it reports no mid-loop compress, moving every particle array
 * with mf_particles_compress_move after a round that does.  The working arrays of a round and the compress plan live in
 * a per-device arena of the library that grows geometrically and never shrinks; a plan stays valid until the next
 * mf_resample_round / mf_particles_compress_plan on that device.
 */
#ifndef MANTA_HIP_RESAMPLE_H
#define MANTA_HIP_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  adjustNumber (rounds, compress, seeding, pdata initialisation), combineGridVel, setBoundNeumann, initFromFlags */
#define MF_RESAMPLE_ABI_VERSION 1
int mf_resample_abi_version(void);

/* Grid<T>::setBoundNeumann -> knSetBoundaryNeumann, grid.cpp:640-669, on one 32-bit plane (Real, int, or one component of a
 * Vec3 grid): every cell within boundaryWidth + 1 of a side takes the value of the nearest cell inside.  Needs
 * sx, sy (and sz in 3-D) >= 2 * boundaryWidth + 3, so that no source cell is itself a boundary cell. */
int mf_grid_set_bound_neumann(int sx, int sy, int sz, void* data, int boundaryWidth, void* stream);

/* LevelsetGrid::initFromFlags, levelset.cpp:231-238: phi = -0.5 on fluid cells (and on obstacle cells with ignoreWalls), else 0.5 */
int mf_levelset_init_from_flags(int64_t n, float* phi, const int32_t* flags, int ignoreWalls, void* stream);

/* combineGridVel -> knCombineVels, plugin/flip.cpp:748-776.  vel, weight, combineVel: MAC / Vec3 grids (SoA); phi nullable.
 * In 2-D the z component goes through the same code. */
int mf_combine_grid_vel(int sx, int sy, int sz, float* vel, const float* weight, float* combineVel, const float* phi,
                        float narrowBand, float thresh, void* stream);

/* One round of adjustNumber's particle loop, plugin/flip.cpp:214-237 with ParticleSystem::kill, particle.h:423-427, over the
 * particles [i0, np): class (out of the domain / phi > 0 / below the band: killed; phi > surfaceLs: kept and counted; else
 * culled when its cell holds more than maxParticles counted particles before it), PDELETE set and `tmp` (int grid, the
 * per-cell counts, zeroed by the caller before the first round) raised up to and including the first particle idx* whose
 * kill makes mDeletes exceed mDeleteChunk; then the compress plan of the whole array (see mf_particles_compress_plan).
 * result_host (4 x int64, valid on return: the call synchronises the stream once):
 *   [0] idx*, or -1 when the round reached np without a compress   [1] kills applied in this round
 *   [2] particles left after the compress (np when [0] is -1)       [3] holes the plan fills (0 when [0] is -1)
 * When [0] >= 0 the caller moves pos, flag and every pdata channel, sets (np, mDeletes, mDeleteChunk) = ([2], 0, [2] / 20)
 * and calls again with i0 = idx* + 1; otherwise mDeletes += [1]. */
int mf_resample_round(int sx, int sy, int sz, const float* phi, int32_t* tmp, int64_t np, int64_t pstride, const float* pos,
                      int32_t* pflag, int64_t i0, int maxParticles, float narrowBand, float surfaceLs, int64_t mDeletes,
                      int64_t mDeleteChunk, int64_t* result_host, void* stream);

/* ParticleSystem::compress, particle.h:614-633, as a plan: with M the number of particles without PDELETE, the k-th deleted
 * slot below M (ascending) takes the k-th kept slot at or above M (descending) -- the serial tail fill.  result_host
 * (2 x int64, one stream synchronise): [0] M, [1] holes. */
int mf_particles_compress_plan(int64_t np, const int32_t* pflag, int64_t* result_host, void* stream);
/* apply the current plan to one array of `ncomp` planes of 32-bit words with component stride pstride (pos, flag, a pdata channel) */
int mf_particles_compress_move(int64_t holes, int ncomp, int64_t pstride, void* data, void* stream);

/* The seeding loop of adjustNumber, plugin/flip.cpp:239-258, first half, and the head of insertBufferedParticles,
 * particle.h:639: clears PNEW on the np particles, then per cell (flat index order) the number of particles to add -- 0 where
 * phi > surfaceLs, where narrowBand > 0 and phi < -narrowBand, where exclude (nullable) < 0, or where the cell is not fluid;
 * else max(minParticles - tmp, 0) -- and their exclusive prefix sum into `offsets` (int grid).  total_host: the sum (one
 * stream synchronise). */
int mf_resample_seed_plan(int sx, int sy, int sz, const int32_t* flags, const float* phi, const float* exclude, const int32_t* tmp,
                          int minParticles, float narrowBand, float surfaceLs, int64_t np, int32_t* pflag, int32_t* offsets,
                          int64_t* total_host, void* stream);
/* second half + insertBufferedParticles, particle.h:642-650: new particle m of the call (m = offsets[cell] + its number in the
 * cell) gets pos = Vec3(i, j, k) + (reals[3m], reals[3m+1], reals[3m+2]) (z = 0.5 in 2-D) and flag PNEW at slot np + m.
 * reals: at least 3 * total values of the call's RandomStream(9832), on the device; pstride >= np + total. */
int mf_resample_seed_insert(int sx, int sy, int sz, const int32_t* offsets, const float* reals, int64_t np, int64_t total,
                            int64_t pstride, float* pos, int32_t* pflag, void* stream);

/* ParticleDataImpl<T>::initNewValue, particle.cpp:348-369, for the particles [first, first + count): mode 0: 0 (no source grid;
 * ncomp planes of 32-bit words), 1: grid.getInterpolated(pos) of a Real (ncomp 1) or Vec3 (ncomp 3) grid, 2: MACGrid::getInterpolated
 * (ncomp 3). */
int mf_pdata_init_new(int sx, int sy, int sz, const float* grid, int mode, int ncomp, int64_t first, int64_t count, int64_t pstride,
                      const float* pos, void* data, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_RESAMPLE_H */
