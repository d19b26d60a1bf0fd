/*
 * manta_hip_turbulence.h -- C ABI extension of `libmanta_hip.so`: the k-epsilon turbulence model of source/plugin/kepsilon.cpp
 * (KEpsilonComputeProduction :38-99, KEpsilonSources :102-126, KEpsilonBcs :129-140, KEpsilonGradientDiffusion :143-179) and the
 * diagnostics of source/plugin/waveletturbulence.cpp that share its centred-velocity stencil (computeVorticity :204-209,
 * computeStrainRateMag :212-236, getCurl :310-316), and the device half of the turbulence particles of source/turbulencepart.cpp
 * (KnSynthesizeTurbulence :79-110, the marking loop of deleteInObstacle :133-138, resetTexCoords :70-76).
 *
 * It lives under include/ext/ because the set of headers include/manta_hip_*.h is frozen (tests/test_extensions_api.py); the rules are
 * those of the other extension headers: include/manta_hip.h and MF_ABI_VERSION stay as they are, a library either implements the whole
 * extension, reporting MF_TURBULENCE_ABI_VERSION through mf_turbulence_abi_version(), or none of it.  Conventions (error plumbing,
 * borrowed device pointers, SoA Vec3 grids, idx = i + sx*(j + sy*k), streams) are those of include/manta_hip.h.  The entries do not
 * know the z-slab window (mf_set_slab_window): grids are whole domains.  Every entry is asynchronous; every scratch array is the
 * caller's.  All of them are bit-identical to the reference built without contraction; DESIGN.md section 14 has the fp32 / fp64 map.
 */
#ifndef MANTA_HIP_TURBULENCE_H
#define MANTA_HIP_TURBULENCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_turbulence_production, mf_turbulence_sources, mf_turbulence_bcs, mf_turbulence_grad_diff, mf_turbulence_strain_mag,
 *      mf_turbulence_vorticity, mf_turbulence_curl_component, mf_turbulence_synthesize, mf_turbulence_mark_in_obstacle,
 *      mf_turbulence_reset_tex */
#define MF_TURBULENCE_ABI_VERSION 1
int mf_turbulence_abi_version(void);

/* KEpsilonComputeProduction in one pass, 3-D grids only.  Every cell: KnTurbulenceClamp (k clamped to [minK, maxK], eps moved so
 * that nu = Cmu k^2 / eps stays inside [1e-3, 5]; both limits from the clamped k and the unclamped eps), k and eps rewritten in place.
 * Interior cells (bnd = 1): prod = 2 nuT S^2 pscale, nuT = Cmu k^2 / eps and, where strain != NULL, strain = sqrt(S^2) from the
 * clamped values, zeros where eps <= 0; border cells of prod / nuT / strain are not written.  The centred velocity of a neighbour is
 * GetCentered's expression evaluated on the fly; a neighbour on a face of the domain is the copy FillInBoundary makes, i.e. the value
 * of the cell itself. */
int mf_turbulence_production(int sx, int sy, int sz, const float* vel, float* k, float* eps, float* prod, float* nuT, float* strain,
                             float pscale, void* stream);

/* KEpsilonSources: KnAddTurbulenceSource (with both pre-clamps) and KnTurbulenceClamp fused, element-wise over n cells */
int mf_turbulence_sources(int64_t n, float* k, float* eps, const float* prod, float dt, void* stream);

/* KEpsilonBcs: k = vk = 1.5 intensity^2, eps = Cmu vk^2 / nu in every cell (fillArea != 0) or in every obstacle cell */
int mf_turbulence_bcs(int64_t n, const int32_t* flags, float* k, float* eps, float intensity, float nu, int fillArea, void* stream);

/* one field of KEpsilonGradientDiffusion: out = f + ((LaplaceOp(f) * nuT) * (dt / sigma)) for `ncomp` scalar planes of n cells each
 * (1: k or eps; 3: the components of a MAC grid, each at its own index with the cell's nuT).  `pass` is the number of fields the
 * reference's one `res` grid went through before this plane's first (k: 0, eps: 1, vel: 2) and coef[0..4] = dt/1, dt/1.3, dt/sigmaU x 3:
 * on a border cell LaplaceOp writes nothing, so `res` there is 0 multiplied through every earlier field's factors (a NaN or infinite
 * nuT shows; a finite one leaves a signed zero).  out must not alias f. */
int mf_turbulence_grad_diff(int sx, int sy, int sz, int ncomp, const float* f, float* out, const float* nuT, int pass, const float* coef,
                            void* stream);

/* computeStrainRateMag: mag = S^2 on the interior (2-D: of the plane); GetCentered without FillInBoundary, so the centred velocity
 * of a border cell is 0.  Border cells of mag are not written. */
int mf_turbulence_strain_mag(int sx, int sy, int sz, const float* vel, float* mag, void* stream);

/* computeVorticity: vorticity = CurlOp(GetCentered(vel)) on the interior, border cells not written; norm (may be NULL) = GridNorm of
 * vorticity over every cell */
int mf_turbulence_vorticity(int sx, int sy, int sz, const float* vel, float* vorticity, float* norm, void* stream);

/* getCurl: vort = component `comp` of CurlOp(GetCentered(vel)); 0 in the border cells */
int mf_turbulence_curl_component(int sx, int sy, int sz, const float* vel, float* vort, int comp, void* stream);

/* KnSynthesizeTurbulence, one thread per slot (deleted slots included, as in the reference).  pos / tex0 / tex1 are particle vectors
 * with component stride pstride.  A slot whose truncated position is outside the grid (2-D: truncated z != 0) is skipped.  Else
 * ks = sqrt(max(k.getInterpolated(pos) - kmin, 0)); per octave vel += alpha * n0 + (1 - alpha) * n1 with n = evaluateCurl(tex *
 * multiplier) * amplitude, both evaluated, amplitude *= 0.56123f, multiplier *= 2, starting from scale * ks and invL0; then pos, tex0
 * and tex1 each += vel * dt.  tile: 3 x 128^3 noise tile; params: the noise parameter block of mf_apply_noise_vec3. */
int mf_turbulence_synthesize(int sx, int sy, int sz, const float* k, const float* tile, const float* params, int64_t np, int64_t pstride,
                             float* pos, float* tex0, float* tex1, float alpha, float dt, int octaves, float scale, float invL0, float kmin,
                             void* stream);

/* the marking loop of TurbulenceParticleSystem::deleteInObstacle: pflag |= MF_PDELETE for every slot whose truncated position is an
 * obstacle cell.  Contract: every position lies inside the grid (the reference reads outside the flag grid otherwise); a slot that
 * does not is left alone here. */
int mf_turbulence_mark_in_obstacle(int sx, int sy, int sz, const int32_t* flags, int64_t np, int64_t pstride, const float* pos, int32_t* pflag,
                                   void* stream);

/* resetTexCoords: tex = pos - inflow for every slot */
int mf_turbulence_reset_tex(int64_t np, int64_t pstride, const float* pos, float* tex, float ix, float iy, float iz, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_TURBULENCE_H */
