// vec3_math.h -- the fp32 Vec3 arithmetic of util/vectorbase.h that the whitewater kernels share: secparts.hip (the combined potentials)
// and gridops.hip (the legacy single-potential plugins).  One definition each; everything keeps the reference's promotion points.
#pragma once
#include "common.h"

// In an inner namespace: the names are generic (dot, norm3, normalized, V3); a user says `using namespace mf::v3;`.
namespace mf {
namespace v3 {

struct V3 {
	float x, y, z;
};
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 v) { return {s * v.x, s * v.y, s * v.z}; }
__device__ __forceinline__ V3 operator/(V3 v, float s) { return {v.x / s, v.y / s, v.z / s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// getNormalized, vectorbase.h:404-416, S = float: |v|^2 in float, the "== 1" test in double, and -- the header's template sees the
// double sqrt only -- fac = (float)(1. / sqrt((double)l)), which is not always (float)(1. / sqrtf(l))
__device__ __forceinline__ V3 normalized(V3 v) {
	const float l = v.x * v.x + v.y * v.y + v.z * v.z;
	const float eps2 = 1e-6f * 1e-6f;
	if (fabs((double)l - 1.) < (double)eps2) return v;
	if (l > eps2) {
		const float fac = (float)(1. / sqrt((double)l));
		return {v.x * fac, v.y * fac, v.z * fac};
	}
	return {0.f, 0.f, 0.f};
}
// norm, vectorbase.h:384-389
__device__ __forceinline__ float norm3(V3 v) {
	const float l = v.x * v.x + v.y * v.y + v.z * v.z;
	const float eps2 = 1e-6f * 1e-6f;
	if (l <= eps2) return 0.f;
	return (fabs((double)l - 1.) < (double)eps2) ? 1.f : sqrtf(l);
}
// std::min(a, b)
__device__ __forceinline__ float std_min(float a, float b) { return (b < a) ? b : a; }
// clampPotential, secondaryparticles.cpp:25-27
__device__ __forceinline__ float clamp_potential(float p, float tmin, float tmax) { return (std_min(p, tmax) - std_min(p, tmin)) / (tmax - tmin); }

}  // namespace v3
}  // namespace mf
