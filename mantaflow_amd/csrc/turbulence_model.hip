// turbulence_model.hip -- the k-epsilon turbulence model (include/ext/manta_hip_turbulence.h): the reference's whole-grid chains of
// source/plugin/kepsilon.cpp fused into one kernel per plugin, and the three diagnostics of plugin/waveletturbulence.cpp that share
// the centred-velocity stencil; the per-particle kernels of the turbulence particle system (turbulencepart.cpp).
// Reference: plugin/kepsilon.cpp, plugin/waveletturbulence.cpp:204-236, 310-316, commonkernels.h, turbulencepart.cpp, noisefield.h.
//
// fp32 / fp64 map: Real is float; a `double` literal promotes the expression it stands in, and the result is
// rounded once where it is stored into a Real.  `0.5 * x` is an exact halving either way (half_of).
#include "common.h"
#include "wavelet_noise_vec.h"
#include "../../include/ext/manta_hip_turbulence.h"
#include <math.h>

using namespace mf;

namespace {

// kepsilon.cpp:24-35: `const Real c = <double literal>`
constexpr float keCmu = (float)0.09, keC1 = (float)1.44, keC2 = (float)1.92;   // keS1 = 1.0 and keS2 = 1.3 reach the library inside coef[]
constexpr float keU0 = (float)1.0, keImin = (float)2e-3, keImax = (float)1.0, keNuMin = (float)1e-3, keNuMax = (float)5.0;

__host__ __device__ __forceinline__ float half_of(float x) { return (float)(0.5 * (double)x); }

// `1.5*square(keU0)*square(x)`: (1.5 * Real) * Real in double, rounded into a const Real
inline float k_limit(float x) { return (float)(1.5 * (double)(keU0 * keU0) * (double)(x * x)); }

// KnTurbulenceClamp, kepsilon.cpp:38-50; clamp() of general.h:137-141 (a NaN passes)
__device__ __forceinline__ void turbulence_clamp(float& ke, float& eps, float minK, float maxK) {
	if (ke < minK) ke = minK;
	else if (ke > maxK) ke = maxK;
	const float c = keCmu * (ke * ke);
	const float nu = c / eps;
	if (nu > keNuMax) eps = c / keNuMax;
	if (nu < keNuMin) eps = c / keNuMin;
}

// GetCentered, commonkernels.h:126-131, at an interior cell q: v = 0.5 * (vel + Vec3(vel(i+1).x, vel(j+1).y, 0)), then
// `v[2] += 0.5 * vel(k+1).z` (a double sum rounded once) in 3-D and v[2] = 0 in 2-D
__device__ __forceinline__ void centered(const Dim& d, const float* __restrict__ vel, int64_t q, float v[3]) {
	const int64_t n = d.n;
	v[0] = half_of(vel[q] + vel[q + 1]);
	v[1] = half_of(vel[n + q] + vel[n + q + d.Y]);
	v[2] = 0.f;
	if (d.is3d) v[2] = (float)((double)half_of(vel[2 * n + q] + 0.f) + 0.5 * (double)vel[2 * n + q + d.Z]);
}
__device__ __forceinline__ bool interior(const Dim& d, int i, int j, int k) { return INTERIOR(d); }
// the centred grid at (i, j, k), a neighbour of an interior cell.  FILL: after FillInBoundary(g = 1), where a cell on a face of the
// domain is the copy of its interior neighbour (an interior cell's neighbours are never edge or corner cells, the only ones whose
// copy depends on the sweep order): the coordinate clamps into the interior.  !FILL: the border of the centred grid is 0.
template <bool FILL>
__device__ __forceinline__ void centered_at(const Dim& d, const float* __restrict__ vel, int i, int j, int k, float v[3]) {
	if (FILL) {
		i = min(max(i, 1), d.sx - 2);
		j = min(max(j, 1), d.sy - 2);
		if (d.is3d) k = min(max(k, 1), d.sz - 2);
	} else if (!interior(d, i, j, k)) {
		v[0] = v[1] = v[2] = 0.f;
		return;
	}
	centered(d, vel, i + d.Y * j + d.Z * k, v);
}

// S^2 of KnComputeProduction :63-71 / KnComputeStrainRateMag :216-229 at the interior cell (i, j, k): three fp32 squares summed in
// fp32, then `+ 2.0 * square(S)` three times in double, rounded once
template <bool FILL>
__device__ __forceinline__ float strain_sq(const Dim& d, const float* __restrict__ vel, int64_t idx, int i, int j, int k) {
	const int64_t n = d.n;
	const float dx = vel[idx + 1] - vel[idx], dy = vel[n + idx + d.Y] - vel[n + idx];
	// production: vel(k+1).z - vel.z; strain magnitude: (0 - vel.z) + vel(k+1).z -- the same fp32 number (the negation is exact)
	const float dz = d.is3d ? (0.f - vel[2 * n + idx]) + vel[2 * n + idx + d.Z] : 0.f;
	float p[3], m[3], ux[3], uy[3], uz[3] = {0.f, 0.f, 0.f};
	centered_at<FILL>(d, vel, i + 1, j, k, p);
	centered_at<FILL>(d, vel, i - 1, j, k, m);
#pragma unroll
	for (int c = 0; c < 3; c++) ux[c] = half_of(p[c] - m[c]);
	centered_at<FILL>(d, vel, i, j + 1, k, p);
	centered_at<FILL>(d, vel, i, j - 1, k, m);
#pragma unroll
	for (int c = 0; c < 3; c++) uy[c] = half_of(p[c] - m[c]);
	if (d.is3d) {
		centered_at<FILL>(d, vel, i, j, k + 1, p);
		centered_at<FILL>(d, vel, i, j, k - 1, m);
#pragma unroll
		for (int c = 0; c < 3; c++) uz[c] = half_of(p[c] - m[c]);
	}
	const float S12 = half_of(ux[1] + uy[0]), S13 = half_of(ux[2] + uz[0]), S23 = half_of(uy[2] + uz[1]);
	const float diag = (dx * dx + dy * dy) + dz * dz;
	return (float)((((double)diag + 2.0 * (double)(S12 * S12)) + 2.0 * (double)(S13 * S13)) + 2.0 * (double)(S23 * S23));
}

// KEpsilonComputeProduction, kepsilon.cpp:86-99: clamp on every cell, production on the interior.  k / eps are rewritten in place:
// no thread reads another cell's k or eps.
__global__ void __launch_bounds__(BLOCK)
k_production(Dim d, const float* __restrict__ vel, float* __restrict__ kg, float* __restrict__ eg, float* __restrict__ prod,
             float* __restrict__ nuT, float* __restrict__ strain, float minK, float maxK, float pscale) {
	CELL_IJK(d)
	float ke = kg[idx], eps = eg[idx];
	turbulence_clamp(ke, eps, minK, maxK);
	kg[idx] = ke;
	eg[idx] = eps;
	if (!INTERIOR(d)) return;
	float P = 0.f, nu = 0.f, st = 0.f;
	if (eps > 0.f) {
		nu = keCmu * (ke * ke) / eps;
		const float S2 = strain_sq<true>(d, vel, idx, i, j, k);
		P = (float)(((2.0 * (double)nu) * (double)S2) * (double)pscale);
		st = sqrtf(S2);
	}
	prod[idx] = P;
	nuT[idx] = nu;
	if (strain) strain[idx] = st;
}

// KnAddTurbulenceSource :102-113 and KnTurbulenceClamp
__global__ void __launch_bounds__(BLOCK)
k_sources(int64_t n, float* __restrict__ kg, float* __restrict__ eg, const float* __restrict__ pg, float dt, float minK, float maxK) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	const float eps = eg[idx], prod = pg[idx];
	float ke = kg[idx];
	if (ke <= 0.f) ke = (float)1e-3;
	float newK = ke + dt * (prod - eps);
	float newEps = eps + dt * (prod * keC1 - eps * keC2) * (eps / ke);
	if (newEps <= 0.f) newEps = (float)1e-4;
	turbulence_clamp(newK, newEps, minK, maxK);
	kg[idx] = newK;
	eg[idx] = newEps;
}

// KEpsilonBcs :129-140
__global__ void __launch_bounds__(BLOCK)
k_bcs(int64_t n, const int32_t* __restrict__ flags, float* __restrict__ kg, float* __restrict__ eg, float vk, float ve, int fillArea) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	if (fillArea || (flags[idx] & MF_OBSTACLE)) {
		kg[idx] = vk;
		eg[idx] = ve;
	}
}

struct Coefs {
	float v[5];
};
// ApplyGradDiff :143-154 and `grid += res`: LaplaceOp, commonkernels.h:75-80 (each line `- 2.0 * grid` in double, stored to fp32,
// the next line added with `+=`: one more double sum rounded once), `res *= nu`, `res *= dt / sigma`, `f += res`; blockIdx.y is
// the scalar plane
__global__ void __launch_bounds__(BLOCK)
k_grad_diff(Dim d, const float* __restrict__ f, float* __restrict__ out, const float* __restrict__ nuT, int pass, Coefs C) {
	CELL_IJK(d)
	const int comp = blockIdx.y;
	f += (int64_t)comp * d.n;
	out += (int64_t)comp * d.n;
	const float nu = nuT[idx], g = f[idx];
	float r;
	if (INTERIOR(d)) {
		r = (float)(((double)f[idx + 1] - 2.0 * (double)g) + (double)f[idx - 1]);
		r = (float)((double)r + (((double)f[idx + d.Y] - 2.0 * (double)g) + (double)f[idx - d.Y]));
		if (d.is3d) r = (float)((double)r + (((double)f[idx + d.Z] - 2.0 * (double)g) + (double)f[idx - d.Z]));
	} else {
		// the reference's one `res` grid: cleared once, never written on the border by LaplaceOp, scaled by every field before
		r = 0.f;
		for (int q = 0; q < pass + comp; q++) r = (r * nu) * C.v[q];
	}
	r = (r * nu) * C.v[pass + comp];
	out[idx] = g + r;
}

// KnComputeStrainRateMag, waveletturbulence.cpp:212-231
__global__ void __launch_bounds__(BLOCK) k_strain_mag(Dim d, const float* __restrict__ vel, float* __restrict__ mag) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	mag[idx] = strain_sq<false>(d, vel, idx, i, j, k);
}

// CurlOp, commonkernels.h:38-47, of the centred velocity (border 0) at the interior cell (i, j, k)
__device__ __forceinline__ void curl_centered(const Dim& d, const float* __restrict__ vel, int i, int j, int k, float v[3]) {
	float xp[3], xm[3], yp[3], ym[3], zp[3], zm[3];
	centered_at<false>(d, vel, i + 1, j, k, xp);
	centered_at<false>(d, vel, i - 1, j, k, xm);
	centered_at<false>(d, vel, i, j + 1, k, yp);
	centered_at<false>(d, vel, i, j - 1, k, ym);
	v[0] = v[1] = 0.f;
	v[2] = half_of((xp[1] - xm[1]) - (yp[0] - ym[0]));
	if (d.is3d) {
		centered_at<false>(d, vel, i, j, k + 1, zp);
		centered_at<false>(d, vel, i, j, k - 1, zm);
		v[0] = half_of((yp[2] - ym[2]) - (zp[1] - zm[1]));
		v[1] = half_of((zp[0] - zm[0]) - (xp[2] - xm[2]));
	}
}
// norm(), vectorbase.h:384-389: fp32 squares; `l - 1.` and the comparison in double; sqrt of a float
__device__ __forceinline__ float norm3(float x, float y, float z) {
	const float l = x * x + y * y + z * z;
	const float eps2 = 1e-6f * 1e-6f;
	if (l <= eps2) return 0.f;
	return (fabs((double)l - 1.) < (double)eps2) ? 1.f : sqrtf(l);
}
// computeVorticity :204-209 (nrm may be NULL) and getCurl :310-316 (COMP >= 0: that component alone, 0 on the border)
__global__ void __launch_bounds__(BLOCK)
k_vorticity(Dim d, const float* __restrict__ vel, float* __restrict__ vort, float* __restrict__ nrm, int comp) {
	CELL_IJK(d)
	const int64_t n = d.n;
	const bool in = INTERIOR(d);
	float v[3] = {0.f, 0.f, 0.f};
	if (in) curl_centered(d, vel, i, j, k, v);
	if (comp >= 0) {
		vort[idx] = v[comp];
		return;
	}
	if (in) {
		vort[idx] = v[0];
		vort[n + idx] = v[1];
		vort[2 * n + idx] = v[2];
	} else if (nrm) {
		v[0] = vort[idx];
		v[1] = vort[n + idx];
		v[2] = vort[2 * n + idx];
	}
	if (nrm) nrm[idx] = norm3(v[0], v[1], v[2]);
}

// ---- turbulence particles, turbulencepart.cpp ----
// WaveletNoiseField::evaluateCurl, noisefield.h:387-394
__device__ __forceinline__ void noise_evaluate_curl(const NoiseParams& P, const float* __restrict__ tile, float x, float y, float z, float cu[3]) {
	float d0[3], d1[3], d2[3];
	noise_evaluate_vec(P, tile, x, y, z, 0, d0);
	noise_evaluate_vec(P, tile, x, y, z, 1, d1);
	noise_evaluate_vec(P, tile, x, y, z, 2, d2);
	cu[0] = d0[1] - d1[2];
	cu[1] = d2[2] - d0[0];
	cu[2] = d1[0] - d2[1];
}
// (int) truncates toward zero, so the truncated coordinate lies in [0, s) exactly when -1 < p < s; a NaN or a value beyond the
// int range (INT_MIN after the reference's conversion) is outside
__device__ __forceinline__ bool trunc_in(float p, int s) { return p > -1.f && p < (float)s; }
// GridBase::isInBounds(toVec3i(pos), 0), grid.h:430-438: a 2-D grid wants the truncated z to be 0
__device__ __forceinline__ bool pos_in_bounds(const Dim& d, float x, float y, float z) {
	return trunc_in(x, d.sx) && trunc_in(y, d.sy) && trunc_in(z, d.is3d ? d.sz : 1);
}

// KnSynthesizeTurbulence, turbulencepart.cpp:79-110: one thread per slot, deleted slots included
__global__ void __launch_bounds__(BLOCK)
k_synthesize(Dim d, const float* __restrict__ kgrid, const float* __restrict__ tile, NoiseParams P, int64_t np, int64_t ps, float* __restrict__ pos,
             float* __restrict__ tex0, float* __restrict__ tex1, float alpha, float dt, int octaves, float scale, float invL0, float kmin) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= np) return;
	const float px = pos[p], py = pos[ps + p], pz = pos[2 * ps + p];
	if (!pos_in_bounds(d, px, py, pz)) return;
	const float k2 = interpol1(d, kgrid, px, py, pz) - kmin;
	const float ks = k2 < 0.f ? 0.f : sqrtf(k2);
	float amplitude = scale * ks, multiplier = invL0;
	float vel[3] = {0.f, 0.f, 0.f};
	const float t0[3] = {tex0[p], tex0[ps + p], tex0[2 * ps + p]}, t1[3] = {tex1[p], tex1[ps + p], tex1[2 * ps + p]};
	const float beta = 1.0f - alpha;
	for (int o = 0; o < octaves; o++) {
		float n0[3], n1[3];
		noise_evaluate_curl(P, tile, t0[0] * multiplier, t0[1] * multiplier, t0[2] * multiplier, n0);
		noise_evaluate_curl(P, tile, t1[0] * multiplier, t1[1] * multiplier, t1[2] * multiplier, n1);
#pragma unroll
		for (int c = 0; c < 3; c++) vel[c] += alpha * (n0[c] * amplitude) + beta * (n1[c] * amplitude);
		amplitude *= 0.56123f;
		multiplier *= 2.0f;
	}
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const float dx = vel[c] * dt;
		pos[c * ps + p] += dx;
		tex0[c * ps + p] = t0[c] + dx;
		tex1[c * ps + p] = t1[c] + dx;
	}
}

// TurbulenceParticleSystem::deleteInObstacle :133-138, the marking loop.  The reference reads flags at the truncated position without
// a bounds check; a slot outside the grid (outside the contract) is "not an obstacle" here
__global__ void __launch_bounds__(BLOCK)
k_mark_in_obstacle(Dim d, const int32_t* __restrict__ flags, int64_t np, int64_t ps, const float* __restrict__ pos, int32_t* __restrict__ pflag) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= np) return;
	const float px = pos[p], py = pos[ps + p], pz = pos[2 * ps + p];
	if (!(trunc_in(px, d.sx) && trunc_in(py, d.sy) && trunc_in(pz, d.sz))) return;
	const int i = (int)px, j = (int)py, k = (int)pz;
	if (flags[i + d.Y * j + (int64_t)d.sx * d.sy * k] & MF_OBSTACLE) pflag[p] |= MF_PDELETE;
}

// resetTexCoords :70-76
__global__ void __launch_bounds__(BLOCK)
k_reset_tex(int64_t np, int64_t ps, const float* __restrict__ pos, float* __restrict__ tex, float ix, float iy, float iz) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= np) return;
	tex[p] = pos[p] - ix;
	tex[ps + p] = pos[ps + p] - iy;
	tex[2 * ps + p] = pos[2 * ps + p] - iz;
}

}  // namespace

extern "C" {

int mf_turbulence_abi_version(void) { return MF_TURBULENCE_ABI_VERSION; }

static int check_particles(const char* who, int64_t np, int64_t pstride) {
	if (np < 0 || pstride < np) return fail("%s: invalid particle count %lld / stride %lld", who, (long long)np, (long long)pstride);
	return 0;
}

int mf_turbulence_synthesize(int sx, int sy, int sz, const float* k, const float* tile, const float* params, int64_t np, int64_t pstride,
                             float* pos, float* tex0, float* tex1, float alpha, float dt, int octaves, float scale, float invL0, float kmin,
                             void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	MF_TRY(check_particles("mf_turbulence_synthesize", np, pstride));
	if (np == 0) return 0;
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_synthesize, dim3(nblk(np)), dim3(BLOCK), 0, (hipStream_t)stream, d, k, tile, noise_params_vec(params), np, pstride, pos,
	                   tex0, tex1, alpha, dt, octaves, scale, invL0, kmin);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_turbulence_mark_in_obstacle(int sx, int sy, int sz, const int32_t* flags, int64_t np, int64_t pstride, const float* pos, int32_t* pflag,
                                   void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	MF_TRY(check_particles("mf_turbulence_mark_in_obstacle", np, pstride));
	if (np == 0) return 0;
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_mark_in_obstacle, dim3(nblk(np)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, np, pstride, pos, pflag);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_turbulence_reset_tex(int64_t np, int64_t pstride, const float* pos, float* tex, float ix, float iy, float iz, void* stream) {
	MF_TRY(check_particles("mf_turbulence_reset_tex", np, pstride));
	if (np == 0) return 0;
	hipLaunchKernelGGL(k_reset_tex, dim3(nblk(np)), dim3(BLOCK), 0, (hipStream_t)stream, np, pstride, pos, tex, ix, iy, iz);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_turbulence_production(int sx, int sy, int sz, const float* vel, float* k, float* eps, float* prod, float* nuT, float* strain,
                             float pscale, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (sz < 2) return fail("KEpsilonComputeProduction: 3-D solvers only");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_production, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, vel, k, eps, prod, nuT, strain,
	                   k_limit(keImin), k_limit(keImax), pscale);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_turbulence_sources(int64_t n, float* k, float* eps, const float* prod, float dt, void* stream) {
	if (n < 0) return fail("mf_turbulence_sources: negative size");
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_sources, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, k, eps, prod, dt, k_limit(keImin), k_limit(keImax));
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_turbulence_bcs(int64_t n, const int32_t* flags, float* k, float* eps, float intensity, float nu, int fillArea, void* stream) {
	if (n < 0) return fail("mf_turbulence_bcs: negative size");
	if (n == 0) return 0;
	const float vk = k_limit(intensity);
	const float ve = keCmu * (vk * vk) / nu;
	hipLaunchKernelGGL(k_bcs, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, flags, k, eps, vk, ve, fillArea);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_turbulence_grad_diff(int sx, int sy, int sz, int ncomp, const float* f, float* out, const float* nuT, int pass, const float* coef,
                            void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if ((ncomp != 1 && ncomp != 3) || pass < 0 || pass + ncomp > 5) return fail("mf_turbulence_grad_diff: invalid ncomp %d / pass %d", ncomp, pass);
	if (f == out) return fail("mf_turbulence_grad_diff: out must not alias f");
	const Dim d = mkdim(sx, sy, sz);
	Coefs C;
	for (int q = 0; q < 5; q++) C.v[q] = coef[q];
	hipLaunchKernelGGL(k_grad_diff, dim3(nblk(d.n), ncomp), dim3(BLOCK), 0, (hipStream_t)stream, d, f, out, nuT, pass, C);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_turbulence_strain_mag(int sx, int sy, int sz, const float* vel, float* mag, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_strain_mag, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, vel, mag);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_turbulence_vorticity(int sx, int sy, int sz, const float* vel, float* vorticity, float* norm, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_vorticity, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, vel, vorticity, norm, -1);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_turbulence_curl_component(int sx, int sy, int sz, const float* vel, float* vort, int comp, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (comp < 0 || comp > 2) return fail("getCurl: component %d", comp);
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_vorticity, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, vel, vort, (float*)nullptr, comp);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
