/*
 * manta_hip_secparts.h -- C ABI extension of `libmanta_hip.so`: the secondary particles (spray, foam, bubbles) of
 * source/plugin/secondaryparticles.cpp (Ihmsen et al.): the trapped-air / wave-crest / kinetic-energy potentials and the neighbour
 * ratio (:24-103), the sampling of new particles in "single" and "multiple" cylinder mode (:105-220), the per-type update in "linear"
 * and "cubic" mode (:225-447), flipDeleteParticlesInObstacle (:450-476), setFlagsFromLevelset and setMACFromLevelset (:512-533).
 *
 * It sits beside include/manta_hip.h and leaves that header (and MF_ABI_VERSION) as it is: a library either implements the whole
 * extension, reporting MF_SECPARTS_ABI_VERSION through mf_secparts_abi_version(), or none of it.  Conventions (error plumbing, borrowed
 * device pointers, SoA Vec3 grids, particle vectors with component stride `pstride`, idx = i + sx*(j + sy*k), streams) are those of
 * include/manta_hip.h.  The entries do not know the z-slab window (mf_set_slab_window): grids are whole domains.  Every scratch array
 * is the caller's; an entry whose last pointer argument before the stream is named *_host synchronises the stream to fill it, every
 * other entry is asynchronous.
 */
#ifndef MANTA_HIP_SECPARTS_H
#define MANTA_HIP_SECPARTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_secparts_potentials, mf_secparts_scan_bytes, mf_secparts_sample_plan, mf_secparts_sample_emit, mf_secparts_update,
 *      mf_secparts_delete_in_obstacle, mf_secparts_flags_from_levelset, mf_secparts_mac_from_levelset */
#define MF_SECPARTS_ABI_VERSION 1
int mf_secparts_abi_version(void);

/* flipComputeSecondaryParticlePotentials, :24-103, bit for bit.  The four outputs are cleared, normal = GradientOp(phi) on the
 * interior (its border cells keep their values), then the (2 radius + 1)^3 gather for every itype cell at least `radius` cells from
 * the sides, neighbours visited x outer, y, z inner.  Two passes: `passes` bit 0 is the streaming pass (clear, gradient, and per
 * cell of the interior the scaled centred velocity -> sv, the unit normal -> sn, the neighbour class -> sc: 0 jtype, 1 other,
 * 2 itype), bit 1 the gather, which reads sv / sn / sc only.  3 is the plugin; 1 and 2 exist for timing.
 *   sv, sn : scratch [3][n];  sc : scratch [n].  Cells outside the interior are not written and not read. */
int mf_secparts_potentials(int sx, int sy, int sz, float* potTA, float* potWC, float* potKE, float* neighborRatio, const int32_t* flags,
                           const float* vel, float* normal, const float* phi, int radius, float tauMinTA, float tauMaxTA, float tauMinWC,
                           float tauMaxWC, float tauMinKE, float tauMaxKE, float scaleFromManta, int itype, int jtype, float* sv,
                           float* sn, int32_t* sc, int passes, void* stream);

/* bytes of `tmp` that mf_secparts_sample_plan needs for `entries` plan entries (host only) */
int mf_secparts_scan_bytes(int64_t entries, int64_t* bytes_host);

/* the order-free statement of the sampling loop, :105-220.  An entry is a cell (multiple = 0; entries = n) or a (cell, cylinder) pair
 * with the cylinders in the reference's x, y, z loop order (multiple = 1; entries = 8 n; entry = 8 idx + 4 xhigh + 2 yhigh + zhigh).
 *   nraw [entries] : int(KE * (k_ta * TA + k_wc * WC) * dt), 0 where the cell is no itype cell
 *   poff [entries] : exclusive scan of max(nraw, 0): the entry's first new particle
 *   roff [entries] : exclusive scan of the reals the entry draws (single: 3 if nraw != 0, plus 4 max(nraw, 0); multiple: 4 max(nraw, 0))
 *   totals_host[0] : new particles, totals_host[1] : reals drawn */
int mf_secparts_sample_plan(int sx, int sy, int sz, int multiple, const int32_t* flags, const float* potTA, const float* potWC,
                            const float* potKE, float k_ta, float k_wc, float dt, int itype, int32_t* nraw, int64_t* poff,
                            int64_t* roff, void* tmp, int64_t tmp_bytes, int64_t* totals_host, void* stream);

/* one thread per new particle m in [0, total): its entry by bisection in poff, then the reference's arithmetic as written, with
 * cos / sin of the azimuth taken in fp64 and rounded once.  reals [nreals]: the window of the mode's random stream that this call
 * consumes.  Writes pos, flag (PSPRAY / PBUBBLE / PFOAM by neighborRatio of the cell), v_sec and l_sec of slot np_old + m; v_sec and
 * l_sec have the component stride of the particle system. */
int mf_secparts_sample_emit(int sx, int sy, int sz, int multiple, const float* vel, const float* potTA, const float* potWC,
                            const float* potKE, const float* neighborRatio, const int32_t* nraw, const int64_t* poff,
                            const int64_t* roff, const float* reals, int64_t nreals, int64_t np_old, int64_t total, int64_t pstride,
                            float* pos, int32_t* pflag, float* v_sec, float* l_sec, float lMin, float lMax, float c_s, float c_b,
                            float dt, void* stream);

/* knFlipUpdateSecondaryParticlesLinear (cubic = 0) / ...Cubic (cubic = 1), :236-423, bit for bit; gravity is already divided by the
 * grid scale, dt is the step in use.  kills_host[0]: particles killed by this call (ParticleSystem::kill's count). */
int mf_secparts_update(int sx, int sy, int sz, int cubic, int64_t np, int64_t pstride, float* pos, int32_t* pflag, float* v_sec,
                       float* l_sec, const float* f_sec, const int32_t* flags, const float* vel, const float* neighborRatio, int radius,
                       float gx, float gy, float gz, float k_b, float k_d, float c_s, float c_b, float dt, int exclude, int antitunneling,
                       int itype, int64_t* kills_host, void* stream);

/* knFlipDeleteParticlesInObstacle, :450-469: active particles outside the grid or in an obstacle / outflow cell are killed */
int mf_secparts_delete_in_obstacle(int sx, int sy, int sz, int64_t np, int64_t pstride, const float* pos, int32_t* pflag,
                                   const int32_t* flags, int64_t* kills_host, void* stream);

/* knSetFlagsFromLevelset, :512-517: flags = itype where phi < 0 and the cell has no `exclude` bit */
int mf_secparts_flags_from_levelset(int64_t n, int32_t* flags, const float* phi, int exclude, int itype, void* stream);

/* knSetMACFromLevelset, :524-528: v = c where phi.getInterpolated(Vec3(i, j, k)) > 0 */
int mf_secparts_mac_from_levelset(int sx, int sy, int sz, float* vel, const float* phi, float cx, float cy, float cz, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_SECPARTS_H */
