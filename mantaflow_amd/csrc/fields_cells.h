// fields_cells.h -- the per-cell bodies of fields.hip as __host__ __device__ functions of (d, idx, i, j, k): the kernels call them with
// one thread per cell, and a stand-alone host program (tools/fields_host_check.hip) calls the same text in a serial loop, where the
// host sanitizers can watch every index.
//
// fp32 / fp64 map: Real is float; a `double` literal promotes the expression it stands in, and the result is
// rounded once where it is stored into a Real.  The library is built with -ffp-contract=off.
#pragma once
#include "common.h"
#include <math.h>

namespace mf {
namespace fields {

#define MF_HD __host__ __device__ __forceinline__

MF_HD bool interior(const Dim& d, int i, int j, int k) { return INTERIOR(d); }

// pow(x, 0.5f) as glibc's powf answers it, up to its last bit: sqrtf (correctly rounded; powf is within 1 ulp of it) with powf's two
// special cases, -0 -> +0 and -inf -> +inf.  A negative x, or a NaN, gives NaN in both.
MF_HD float pow_half(float x) {
	if (x == 0.f) return 0.f;
	if (x == -INFINITY) return INFINITY;
	return sqrtf(x);
}

struct Burn {
	float burningRate, flameSmoke, ignitionTemp, maxTemp, dt, cx, cy, cz;
};
// KnProcessBurn, fire.cpp:22-64, at an interior cell
MF_HD void process_burn(int64_t idx, float* fuel, float* density, float* react, float* red, float* green, float* blue, float* heat,
                        const Burn& B) {
	const float origFuel = fuel[idx], origSmoke = density[idx];
	float flame = 0.0f;
	float f = origFuel - B.burningRate * B.dt;
	if (f < 0.0f) f = 0.0f;
	fuel[idx] = f;
	if (origFuel > 1e-6f) {
		const float r = react[idx] * (f / origFuel);
		react[idx] = r;
		flame = pow_half(r);
	} else {
		react[idx] = 0.0f;
	}
	// `(origFuel < 1.0f) ? (1.0 - origFuel) * 0.5f : 0.0f`: a double expression, rounded once into the Real
	float smokeEmit = (origFuel < 1.0f) ? (float)((1.0 - (double)origFuel) * 0.5) : 0.0f;
	smokeEmit = (smokeEmit + 0.5f) * (origFuel - f) * 0.1f * B.flameSmoke;
	const float dens = origSmoke + smokeEmit;
	density[idx] = dens;                      // clamp(density, 0, 1) returns by value and the result is dropped (general.h:137-141)
	if (heat && flame) heat[idx] = (1.0f - flame) * B.ignitionTemp + flame * B.maxTemp;    // a NaN flame is "true"
	if (smokeEmit > 1e-6f) {
		const float smokeFactor = dens / (origSmoke + smokeEmit);
		if (red) red[idx] = (red[idx] + B.cx * smokeEmit) * smokeFactor;
		if (green) green[idx] = (green[idx] + B.cy * smokeEmit) * smokeFactor;
		if (blue) blue[idx] = (blue[idx] + B.cz * smokeEmit) * smokeFactor;
	}
}

// KnUpdateFlame, fire.cpp:78-85
MF_HD float update_flame(float react) { return react > 0.0f ? pow_half(react) : 0.0f; }

// `-4.*v + v(i-1) + v(i+1) + v(j-1) + v(j+1)` (waves.cpp:35, :78 with its `1.*` factors): left to right in double
MF_HD double five_point(const Dim& d, const float* __restrict__ v, int64_t idx) {
	return (((-4. * (double)v[idx] + (double)v[idx - 1]) + (double)v[idx + 1]) + (double)v[idx - d.Y]) + (double)v[idx + d.Y];
}

// the FOR_IJK loop of cgSolveWE, waves.cpp:110-116, and MakeRhsWE :72-80 over a cleared rhs
MF_HD void wave_system(const Dim& d, int64_t idx, bool in, float* A0, float* Ai, float* Aj, float* Ak, float* rhs,
                       const float* __restrict__ ut, const float* __restrict__ utm1, float s, int crankNic) {
	Ai[idx] *= s;
	Aj[idx] *= s;
	Ak[idx] *= s;
	const float a = A0[idx] * s;
	A0[idx] = (float)((double)a + 1.);
	float r = 0.f;
	if (in) {
		r = (float)(2. * (double)ut[idx] - (double)utm1[idx]);
		if (crankNic) r = (float)((double)r + (double)s * five_point(d, ut, idx));
	}
	rhs[idx] = r;
}

// one cell of pass d of extrapolSimpleFlagsHelper<T>, waveletturbulence.cpp:270-289.  T = float (ncomp planes) or int32_t.
template <class T>
MF_HD void extrapolate_cell(const Dim& d, int64_t idx, const int32_t* flags, int32_t* tmp, T* val, int ncomp, int dist, int flagTo) {
	if (tmp[idx] != 0) return;
	if (!(flags[idx] & flagTo)) return;
	const int64_t off[6] = {1, -1, d.Y, -d.Y, d.Z, -d.Z};
	const int nn = d.is3d ? 6 : 4;
	int nbs = 0;
	T sum[3] = {0, 0, 0};
	for (int q = 0; q < nn; q++) {
		const int64_t p = idx + off[q];
		if (tmp[p] == dist) {
			for (int c = 0; c < ncomp; c++) sum[c] += val[(int64_t)c * d.n + p];
			nbs++;
		}
	}
	if (nbs > 0) {
		tmp[idx] = dist + 1;
		for (int c = 0; c < ncomp; c++) val[(int64_t)c * d.n + idx] = sum[c] / (T)nbs;
	}
}

}  // namespace fields
}  // namespace mf
