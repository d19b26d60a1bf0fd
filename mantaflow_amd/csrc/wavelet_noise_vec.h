// wavelet_noise_vec.h -- the evaluation of the wavelet noise field: the scalar form (WaveletNoiseField::evaluate, noisefield.h:163-196,
// 313-336; densityInflow and addNoise in noise.hip, setNoisePdata in grid4d.hip) and the vector form (evaluateVec / evaluateCurl,
// noisefield.h:210-310, 358-394; applyNoiseVec3 in turbulence.hip, the turbulence particles in turbulence_model.hip, setNoisePdataVec3).
#pragma once
#include "common.h"
#include <math.h>

namespace mf {

struct NoiseParams {
	float gsInv[3], seedOff[3], time, posScale[3], posOffset[3], valOffset, valScale, clamp, clampNeg, clampPos;
};
// WNoise, noisefield.h:163-196: quadratic B-spline over the 27 neighbouring tile entries, x fastest
static __device__ __forceinline__ float wnoise(float p0, float p1, float p2, const float* __restrict__ data) {
	float w[3][3];
	int mid[3];
	const float p[3] = {p0, p1, p2};
#pragma unroll
	for (int c = 0; c < 3; c++) {
		mid[c] = (int)ceilf(p[c] - 0.5f);
		const float t = (float)mid[c] - (p[c] - 0.5f);
		w[c][0] = t * t * 0.5f;
		w[c][2] = (1.f - t) * (1.f - t) * 0.5f;
		w[c][1] = 1.f - w[c][0] - w[c][2];
	}
	float result = 0.f;
#pragma unroll
	for (int z = -1; z <= 1; z++)
#pragma unroll
		for (int y = -1; y <= 1; y++)
#pragma unroll
			for (int x = -1; x <= 1; x++) {
				float weight = 1.0f;
				weight *= w[0][x + 1];
				weight *= w[1][y + 1];
				weight *= w[2][z + 1];
				const int xC = (mid[0] + x) & 127, yC = (mid[1] + y) & 127, zC = (mid[2] + z) & 127;
				result += weight * data[(zC * 128 + yC) * 128 + xC];
			}
	return result;
}
// WaveletNoiseField::evaluate, noisefield.h:313-336
static __device__ __forceinline__ float noise_evaluate(const NoiseParams& P, const float* __restrict__ tile, float x, float y, float z) {
	float pos[3] = {x, y, z};
#pragma unroll
	for (int c = 0; c < 3; c++) pos[c] *= P.gsInv[c];
#pragma unroll
	for (int c = 0; c < 3; c++) pos[c] += P.seedOff[c];
#pragma unroll
	for (int c = 0; c < 3; c++) pos[c] += P.time;
#pragma unroll
	for (int c = 0; c < 3; c++) pos[c] *= P.posScale[c];
#pragma unroll
	for (int c = 0; c < 3; c++) pos[c] += P.posOffset[c];
	float v = wnoise(pos[0], pos[1], pos[2], tile);
	v += P.valOffset;
	v *= P.valScale;
	if (P.clamp != 0.f) {
		if (v < P.clampNeg) v = P.clampNeg;
		if (v > P.clampPos) v = P.clampPos;
	}
	return v;
}
// WNoiseVec, noisefield.h:210-310
static __device__ void wnoise_vec(float p0, float p1, float p2, const float* __restrict__ data, float out[3]) {
	const float p[3] = {p0, p1, p2};
	int mid[3];
	float t[3], w[3][3], dw[3][3], nb[3][3][3];
#pragma unroll
	for (int c = 0; c < 3; c++) {
		mid[c] = (int)ceil((double)(p[c] - 0.5f));
		t[c] = (float)mid[c] - (p[c] - 0.5f);
	}
#pragma unroll
	for (int z = -1; z <= 1; z++)
#pragma unroll
		for (int y = -1; y <= 1; y++)
#pragma unroll
			for (int x = -1; x <= 1; x++) {
				const int xC = (mid[0] + x) & 127, yC = (mid[1] + y) & 127, zC = (mid[2] + z) & 127;
				nb[x + 1][y + 1][z + 1] = data[zC * 128 * 128 + yC * 128 + xC];
			}
#pragma unroll
	for (int c = 0; c < 3; c++) {
		dw[c][0] = -t[c];
		dw[c][2] = (1.f - t[c]);
		dw[c][1] = 2.0f * t[c] - 1.0f;
		w[c][0] = t[c] * t[c] * 0.5f;
		w[c][2] = (1.f - t[c]) * (1.f - t[c]) * 0.5f;
		w[c][1] = 1.f - w[c][0] - w[c][2];
	}
#pragma unroll
	for (int comp = 0; comp < 3; comp++) {
		float result = 0.0f;
#pragma unroll
		for (int z = -1; z <= 1; z++)
#pragma unroll
			for (int y = -1; y <= 1; y++)
#pragma unroll
				for (int x = -1; x <= 1; x++) {
					const float a = (comp == 0) ? dw[0][x + 1] : w[0][x + 1];
					const float b = (comp == 1) ? dw[1][y + 1] : w[1][y + 1];
					const float c = (comp == 2) ? dw[2][z + 1] : w[2][z + 1];
					const float weight = a * b * c;
					result += weight * nb[x + 1][y + 1][z + 1];
				}
		out[comp] = result;
	}
}
// WaveletNoiseField::evaluateVec, noisefield.h:338-364
static __device__ void noise_evaluate_vec(const NoiseParams& P, const float* __restrict__ tile, float x, float y, float z, int t, float v[3]) {
	float pos[3] = {x, y, z};
#pragma unroll
	for (int c = 0; c < 3; c++) pos[c] *= P.gsInv[c];
#pragma unroll
	for (int c = 0; c < 3; c++) pos[c] += P.seedOff[c];
#pragma unroll
	for (int c = 0; c < 3; c++) pos[c] += P.time;
#pragma unroll
	for (int c = 0; c < 3; c++) pos[c] *= P.posScale[c];
#pragma unroll
	for (int c = 0; c < 3; c++) pos[c] += P.posOffset[c];
	wnoise_vec(pos[0], pos[1], pos[2], tile + (int64_t)t * 128 * 128 * 128, v);
#pragma unroll
	for (int c = 0; c < 3; c++) v[c] += P.valOffset;
#pragma unroll
	for (int c = 0; c < 3; c++) v[c] *= P.valScale;
	if (P.clamp != 0.f) {
#pragma unroll
		for (int c = 0; c < 3; c++) {
			if (v[c] < P.clampNeg) v[c] = P.clampNeg;
			if (v[c] > P.clampPos) v[c] = P.clampPos;
		}
	}
}
// the leading 18 floats of the host layer's noise parameter block (scene.NoiseField._params)
static inline NoiseParams noise_params_vec(const float* params) {
	NoiseParams P;
	for (int c = 0; c < 3; c++) {
		P.gsInv[c] = params[c];
		P.seedOff[c] = params[3 + c];
		P.posScale[c] = params[7 + c];
		P.posOffset[c] = params[10 + c];
	}
	P.time = params[6];
	P.valOffset = params[13];
	P.valScale = params[14];
	P.clamp = params[15];
	P.clampNeg = params[16];
	P.clampPos = params[17];
	return P;
}

}  // namespace mf
