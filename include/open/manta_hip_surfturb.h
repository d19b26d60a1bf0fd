/*
 * manta_hip_surfturb.h -- C ABI extension of `libmanta_hip.so`: surface turbulence (Mercier et al., "Surface Turbulence for
 * Particle-Based Liquid Simulations"), the stages of
 *   particleSurfaceTurbulence   source/plugin/surfaceturbulence.cpp:1028-1159
 *   debugCheckParts             source/plugin/surfaceturbulence.cpp:1164-1171
 * A point set is pos[3][cap], flag[cap] (ParticleBase::PNEW = 1, PDELETE = 1 << 10); a channel is [ncomp][cap] of the same stride.
 *
 * The rules are those of the other extension headers: include/manta_hip.h and MF_ABI_VERSION stay as they are; a library implements
 * the whole extension, reporting MF_SURFTURB_ABI_VERSION through mf_surfturb_abi_version(), or none of it.  Conventions (error plumbing,
 * borrowed device pointers, SoA, streams) are those of include/manta_hip.h.  Every device entry refuses a z-slab window
 * (mf_set_slab_window).  DESIGN.md section 27 has the contract, the quirks that are kept and the fp32 / fp64 map.
 *
 * `par_host` is the block of 32 floats that mf_surfturb_params writes.  A cell list of resolution R is start[R^3 + 1], ids[n]: the
 * slots of cell c = (i * R + j) * R + k are ids[start[c] .. start[c + 1]) in ascending order, deleted slots included.  A query visits
 * the cells i outer, j, k inner, then the slots ascending, and skips the slots deleted at query time: this is the fp32 summation order
 * of every accumulation.  All per-point passes run over every slot [0, n), deleted ones with their stored positions.
 */
#ifndef MANTA_HIP_SURFTURB_H
#define MANTA_HIP_SURFTURB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against */
#define MF_SURFTURB_ABI_VERSION 1
int mf_surfturb_abi_version(void);

/* Host: the derived parameters of :1086-1092 with the C library's expf / logf / powf and the reference's types, cosf(theta) of
 * seedWaves for this frameCount, and the two radii that are double expressions rounded once.  par_host[32]: res, outerRadius,
 * innerRadius, meanFineDistance, constraintA, normalRadius, tangentRadius, bndm, bndp, dt, waveSpeed, waveDamping, waveSeedFrequency,
 * waveMaxAmplitude, waveMaxFrequency, waveMaxSeedingAmplitude, curvature centre, curvature radius, seed step, cos(theta),
 * Real(meanFineDistance - 1e-6), Real(0.67 * meanFineDistance), dtheta, zeros.  res_host[2] = the resolutions of the coarse and the
 * surface cell list, int(2.f * res / outerRadius) and int(1.f * res / (2.f * meanFineDistance)). */
int mf_surfturb_params(int res, float outerRadius, int surfaceDensity, float dt, float waveSpeed, float waveDamping, float waveSeedFrequency,
                       float waveMaxAmplitude, float waveMaxFrequency, float waveMaxSeedingAmplitude, float curvCenter, float curvRadius,
                       float seedStep, int frameCount, float* par_host, int32_t* res_host);

/* Host: the direction table of initFines (:378-382) in its order, i then phi, with the float sin / cos overloads and the fp32 running
 * phi.  *count_host = the number of directions; dirs_host[cap][3] receives them when cap >= count (dirs_host may be null otherwise). */
int mf_surfturb_directions(const float* par_host, int64_t cap, float* dirs_host, int64_t* count_host);

/* *bytes_host = the size of `tmp` that serves every entry below for point sets of at most n slots, cell lists of at most ncells
 * cells and scans of at most nscan elements.  Touches no device memory. */
int mf_surfturb_tmp_bytes(int64_t n, int64_t ncells, int64_t nscan, int64_t* bytes_host);

/* The cell list of the n positions pos[3][cap]: cell of a point clamp(int(floor(p.c / res * R)), 0, R - 1) per axis in fp32, with the
 * x86 conversion (NaN and values outside int's range land in cell 0 after the clamp).  A stable sort of the slots by cell. */
int mf_surfturb_cells(const float* par_host, int R, int64_t n, int64_t cap, const float* pos, int32_t* start, int32_t* ids, void* tmp,
                      int64_t tmp_bytes, void* stream);

/* initFines as a pass over (coarse particle, direction): mark[p * ndirs + d] = 1 where a surface point is created, then the inclusive
 * scan of mark in place; *total_host = the number of points (one 4-byte read-back).  gridflags is the FlagGrid of sx * sy * sz cells.
 * Precondition: the coarse particles sit in cells [1, size - 2]. */
int mf_surfturb_init_plan(const float* par_host, int sx, int sy, int sz, const int32_t* gridflags, int Rc, const int32_t* cstart,
                          const int32_t* cids, int64_t nc, int64_t ccap, const float* cpos, const int32_t* cflag, int64_t ndirs,
                          const float* dirs, int32_t* mark, void* tmp, int64_t tmp_bytes, int64_t* total_host, void* stream);
/* ... and the points, in the order particle, then direction, into pos[3][cap] with flag 0. */
int mf_surfturb_init_fill(const float* par_host, int64_t nc, int64_t ccap, const float* cpos, int64_t ndirs, const float* dirs,
                          const int32_t* mark, int64_t cap, float* pos, int32_t* flag, void* stream);

/* advectSurfacePoints (:407-432) over the active slots; (Rc, pstart, pids) is the list over prev[3][pcap], in which every slot counts as
 * active; cflag are the coarse particles' flags (PNEW and PDELETE ones are skipped). */
int mf_surfturb_advect(const float* par_host, int Rc, const int32_t* pstart, const int32_t* pids, int64_t nc, int64_t ccap, const float* cpos,
                       const int32_t* cflag, int64_t pcap, const float* prev, int64_t n, int64_t cap, float* pos, const int32_t* flag,
                       void* stream);

/* The add pass of addDeleteSurfacePoints (:566-602) over every slot: cand[3][n] receives the creation positions, mark[n] the
 * inclusive scan of "is buffered"; *total_host = the number of buffered points (one read-back).  Order-free: the lists are static. */
int mf_surfturb_add_plan(const float* par_host, int Rc, const int32_t* cstart, const int32_t* cids, int64_t nc, int64_t ccap,
                         const float* cpos, const int32_t* cflag, int Rs, const int32_t* sstart, const int32_t* sids, int64_t n, int64_t cap,
                         const float* pos, const int32_t* flag, float* cand, int32_t* mark, void* tmp, int64_t tmp_bytes,
                         int64_t* total_host, void* stream);
/* insertBufferedParticles: PNEW is cleared on the n old slots, the `total` buffered points of the plan are appended in ascending
 * source order with flag PNEW (n + total <= cap).  The caller zeroes the channels of the new slots. */
int mf_surfturb_add_apply(int64_t n, int64_t total, int64_t cap, float* pos, int32_t* flag, const float* cand, const int32_t* mark, void* stream);

/* One round of delete pass 1 (:611-618), the serial greedy rule stated order-free: state 0 undecided, 1 kept, 2 killed; a slot
 * outside the domain is killed at once, any other slot is decided once every lower listed neighbour within Real(0.67 d) that was
 * active before the pass is decided -- killed if one of those is kept or a higher listed active neighbour is in range.  Reads
 * state_in (zeroed here when `first`), writes state_out (all n slots); *undecided_host = 1 while a slot is undecided (one read-back).  The list holds the first
 * `listed` slots only by construction (appended points are tested, never seen).  head is 256 bytes of device scratch. */
int mf_surfturb_greedy_round(const float* par_host, int Rs, const int32_t* sstart, const int32_t* sids, int64_t n, int64_t cap,
                             const float* pos, const int32_t* flag, int first, int32_t* state_in, int32_t* state_out, int32_t* head,
                             int32_t* undecided_host, void* stream);
/* The kills of the three delete passes over every slot: state == 2, no active coarse particle within 2 outerRadius, constraint level
 * outside [-0.2, 1.2].  kills_host[3] = the kill calls per pass (a slot already deleted counts again). */
int mf_surfturb_delete(const float* par_host, int Rc, const int32_t* cstart, const int32_t* cids, int64_t nc, int64_t ccap, const float* cpos,
                       const int32_t* cflag, int64_t n, int64_t cap, const float* pos, int32_t* flag, const int32_t* state, int32_t* head,
                       int32_t* kills_host, void* stream);
/* flag &= ~PNEW on n slots (the second insertBufferedParticles of an iteration, which has nothing buffered) */
int mf_surfturb_clear_new(int64_t n, int32_t* flag, void* stream);

/* computeSurfaceNormals and smoothSurfaceNormals (:467-555) into normals[3][cap]; tempv[3][n] is scratch. */
int mf_surfturb_normals(const float* par_host, int Rc, const int32_t* cstart, const int32_t* cids, int64_t nc, int64_t ccap, const float* cpos,
                        const int32_t* cflag, int Rs, const int32_t* sstart, const int32_t* sids, int64_t n, int64_t cap, const float* pos,
                        const int32_t* flag, float* normals, float* tempv, void* stream);
/* regularizeSurfacePoints (:648-723); tempf[n], tempv[3][n] are scratch.  The list stays that of the positions before the call. */
int mf_surfturb_regularize(const float* par_host, int Rs, const int32_t* sstart, const int32_t* sids, int64_t n, int64_t cap, float* pos,
                           const int32_t* flag, const float* normals, float* tempf, float* tempv, void* stream);
/* constrainSurface (:726-738) */
int mf_surfturb_constrain(const float* par_host, int Rc, const int32_t* cstart, const int32_t* cids, int64_t nc, int64_t ccap,
                          const float* cpos, const int32_t* cflag, int64_t n, int64_t cap, float* pos, void* stream);
/* surfaceWaves (:1002-1018): the seven passes on the channels H, DtH, source, seed, seedAmp (each [cap]). */
int mf_surfturb_waves(const float* par_host, int Rs, const int32_t* sstart, const int32_t* sids, int64_t n, int64_t cap, const float* pos,
                      const int32_t* flag, const float* normals, float* H, float* DtH, float* source, float* seed, float* seedAmp,
                      float* tempf, float* tempv, void* stream);

/* prev = pos on the coarse particles without PNEW and PDELETE (:1138-1144) */
int mf_surfturb_save_prev(int64_t nc, int64_t ccap, const float* cpos, const int32_t* cflag, int64_t pcap, float* prev, void* stream);
/* The displaced points (:1147-1152): mark[n] = the inclusive scan of "not deleted", *total_host their number (one read-back) ... */
int mf_surfturb_displaced_plan(int64_t n, const int32_t* flag, int32_t* mark, void* tmp, int64_t tmp_bytes, int64_t* total_host, void* stream);
/* ... and out[3][ocap] = pos + normals * H in slot order, oflag = 0. */
int mf_surfturb_displaced_fill(int64_t n, int64_t cap, const float* pos, const int32_t* flag, const float* normals, const float* H,
                               const int32_t* mark, int64_t ocap, float* out, int32_t* oflag, void* stream);

/* debugCheckParts: *bad_host = the first slot whose toVec3i(pos) is outside the grid, -1 if none (one read-back).  head: 256 bytes. */
int mf_surfturb_check_parts(int sx, int sy, int sz, int64_t n, int64_t cap, const float* pos, int32_t* head, int64_t* bad_host, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_SURFTURB_H */
