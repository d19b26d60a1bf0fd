/*
 * manta_hip_reinit.h -- C ABI extension of `libmanta_hip.so`: level-set reinitialisation by fast marching.
 *   doReinitMarch / LevelsetGrid::reinitMarching   source/levelset.cpp:32-85, 122-228
 *   FastMarch, SetLevelsetBoundaries               source/fastmarch.cpp:23-221, source/fastmarch.h
 * reinitMarching is mf_reinit_march(dir = -1), mf_reinit_set_uninitialized(-maxTime - 1), mf_reinit_march(dir = +1),
 * mf_reinit_set_uninitialized(maxTime + 1).  A march pops the heap in rounds of mutually distant cells and is bit-identical to the
 * reference's serial loop; when it cannot prove that for its input it redoes the march with the literal loop on the host.
 *
 * The rules are those of the other extension headers: include/manta_hip.h and MF_ABI_VERSION stay as they are; a library implements
 * the whole extension, reporting MF_REINIT_ABI_VERSION through mf_reinit_abi_version(), or none of it.  Conventions (error plumbing,
 * borrowed device pointers, SoA, idx = i + sx*(j + sy*k), streams) are those of include/manta_hip.h.  Grids are 3-D with every edge
 * >= 3, or 2-D (sz == 1) with sx, sy >= 3; every device entry refuses a z-slab window (mf_set_slab_window).  DESIGN.md section 18 has
 * the contract, the fp32 / fp64 map and the proof.
 */
#ifndef MANTA_HIP_REINIT_H
#define MANTA_HIP_REINIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_reinit_march, mf_reinit_set_uninitialized, mf_reinit_march_serial */
#define MF_REINIT_ABI_VERSION 1
int mf_reinit_abi_version(void);

/* One march on phi (in place): InitFmIn (dir = -1) or InitFmOut (dir = +1) with ignoreWalls / obstacleType, the seeding loop of
 * doReinitMarch (for dir = +1 the one that correctOuterLayer selects), performMarching up to maxTime, SetLevelsetBoundaries.  vel (MAC
 * grid, SoA [3][n]) is the velocity to transport; the reference transports on the outward march only, so it is read for dir = +1 and may
 * be null.  Scratch, n entries each, contents irrelevant on entry: fm (the FastMarch flags: 0, 1 = FlagInited, 2 = FlagIsOnHeap), key (the
 * time at which a cell went on the heap, 0 where it never did), list, sel, epoch, snapPhi, snapFm, and snapVel [3][n] (null when vel is); ctr = 8
 * ints.  fm and key are left as the march ends and fm is what mf_reinit_set_uninitialized reads.  serial != 0 runs the literal loop on the
 * host at once.  stats_host[6] = windows, sub-rounds, pops, 1 if the serial loop ran, kernel launches, scalar read-backs (windows and
 * sub-rounds are 0 when the serial loop ran).  Synchronises the stream. */
int mf_reinit_march(int sx, int sy, int sz, float* phi, const int32_t* flags, float* vel, int32_t* fm, float* key, int32_t* list, int32_t* sel,
                    int32_t* epoch, float* snapPhi, int32_t* snapFm, float* snapVel, int32_t* ctr, float maxTime, int dir, int ignoreWalls, int correctOuterLayer,
                    int obstacleType, int serial, int64_t* stats_host, void* stream);

/* SetUninitialized: interior cells whose fm is not FlagInited (and, with ignoreWalls, that are not of obstacleType) take val. */
int mf_reinit_set_uninitialized(int sx, int sy, int sz, float* phi, const int32_t* fm, const int32_t* flags, float val, int ignoreWalls,
                                int obstacleType, void* stream);

/* The literal serial march on HOST arrays that InitFmIn / InitFmOut has been applied to: seeding loop, performMarching with a binary heap
 * ordered as the reference's, SetLevelsetBoundaries.  key is n entries of output (as above); *pops_host = number of pops.  Touches no
 * device memory. */
int mf_reinit_march_serial(int sx, int sy, int sz, float* phi, int32_t* fm, float* key, const int32_t* flags, float* vel, float maxTime, int dir,
                           int ignoreWalls, int correctOuterLayer, int obstacleType, int64_t* pops_host);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_REINIT_H */
