/*
 * manta_hip_vortex.h -- C ABI extension of `libmanta_hip.so`: vortex particles.
 *   VortexKernel, KnVpAdvectSelf, KnVpAdvectMesh    source/vortexpart.cpp:24-84
 *   integratePointSet                               source/util/integrator.h:26-78
 *   VPseedK41, densityFromLevelset                  source/plugin/vortexplugins.cpp:169-189, 298-310
 * Targets are caller-owned device arrays pos[3][tcap], flag[tcap]; sources are pos[3][scap], flag[scap], vorticity[3][scap],
 * sigma[scap].  The vortex sheet half of the reference (VortexSheetMesh and its plugins) has no entry here.
 *
 * The rules are those of the other extension headers: include/manta_hip.h and MF_ABI_VERSION stay as they are; a library implements
 * the whole extension, reporting MF_VORTEX_ABI_VERSION through mf_vortex_abi_version(), or none of it.  Conventions (error plumbing,
 * borrowed device pointers, SoA, idx = i + sx*(j + sy*k), streams) are those of include/manta_hip.h.  DESIGN.md section 21 has the
 * fp32 / fp64 map of the velocity sum and the reason it runs in source order.
 */
#ifndef MANTA_HIP_VORTEX_H
#define MANTA_HIP_VORTEX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_vortex_scratch_bytes, mf_vortex_velocity, mf_vortex_integrate, mf_vortex_density_from_levelset, mf_vortex_seed_k41 */
#define MF_VORTEX_ABI_VERSION 1
int mf_vortex_abi_version(void);

/* *bytes_host = the size of `tmp` that mf_vortex_velocity and mf_vortex_integrate need for nS sources (what depends on a source alone
 * is computed into it once per call).  Touches no device memory. */
int mf_vortex_scratch_bytes(int64_t nS, int64_t* bytes_host);

/* One evaluation of the induced velocity: for every target t < nT
 *   u[t] = 0                                                   if tflag[t] & tmask
 *   u[t] = the sum over the sources s = 0 .. nS-1, in that order, of VortexKernel's term (sources with PDELETE skipped)   else
 * accumulated in fp32 without contraction, one thread per target.  tmask is PDELETE (1 << 10) for particles as targets and
 * Mesh::NfFixed (1) for mesh nodes.  `scale` is the reference's scale * dt.  u is [3][ucap], written for t < nT only.  The
 * targets may be the sources (tpos == spos).  Asynchronous. */
int mf_vortex_velocity(int64_t nT, int64_t tcap, const float* tpos, const int32_t* tflag, int tmask, int64_t nS, int64_t scap,
                       const float* spos, const int32_t* sflag, const float* vorticity, const float* sigma, float scale, void* tmp,
                       int64_t tmp_bytes, int64_t ucap, float* u, void* stream);

/* integratePointSet around that sum, one launch per Runge-Kutta stage with the position update fused: integrationMode 0 Euler, 1 RK2,
 * 2 RK4 exactly as written (RK4 with the fork's `uTotal += u`, i.e. x0 + float(1./6.) * (2 u1 + 2 u2 + 2 u3 + u4)).  A stage reads the
 * positions of the stage before and writes the other buffer, so no thread sees a position of its own stage.
 *   spos == tpos: the targets are the sources (advectSelf) and move with the stages; then nS == nT and scap == tcap
 *   otherwise:    the sources stay where they are (applyToMesh)
 * pos2, x0 and uTotal are scratch of [3][tcap] floats each; the result is in tpos on return.  Targets with tflag & tmask go through
 * the same arithmetic with u = 0.  Nothing is read back.  Asynchronous. */
int mf_vortex_integrate(int64_t nT, int64_t tcap, float* tpos, const int32_t* tflag, int tmask, int64_t nS, int64_t scap,
                        const float* spos, const int32_t* sflag, const float* vorticity, const float* sigma, float scale,
                        int integrationMode, float* pos2, float* x0, float* uTotal, void* tmp, int64_t tmp_bytes, void* stream);

/* densityFromLevelset, one thread per cell: 0 in the two outermost layers of every axis (on a 2-D grid that is every cell, as in the
 * reference), value where phi < -sigma, 0 where phi > sigma, else clamp(float(0.5 * value / sigma * (1.0 - phi)), 0, value) with the
 * factor in fp64.  Refuses a z-slab window. */
int mf_vortex_density_from_levelset(int sx, int sy, int sz, const float* phi, float* density, float value, float sigma, void* stream);

/* HOST entry: the C library's half of VPseedK41 for m accepted cells.  p[m] and dir[m][3] are the draws; sigmaOut[m] =
 * float(pow((1.0 - p) * s0 + p * s1, 1. / (-N + 1.0))) with s0, s1 = powf(sigma0 | sigma1, float(-N + 1.0)), and vortOut[m][3] =
 * normalize(dir) * strength * powf(sigma, float(-10./6. + N / 2.0)).  Touches no device. */
int mf_vortex_seed_k41(int64_t m, float strength, float sigma0, float sigma1, float N, const float* p, const float* dir, float* sigmaOut,
                       float* vortOut);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_VORTEX_H */
