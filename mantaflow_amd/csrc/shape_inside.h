// shape_inside.h -- Shape::isInside of the three analytic shapes and the (kind, 12 floats) record they travel in: one definition for
// surface.hip (mf_shape_apply_to_grid) and movingobs.hip (the flag pass of MovingObstacle::moveLinear).  The layout of the 12 floats is
// that of mf_shape_levelset, include/manta_hip.h.
#pragma once
#include "common.h"

namespace mf {

struct ShapeParams {
	float q[12];
};

/* Box::isInside :151-154 (z is tested in 2-D as well), Sphere::isInside :240-242, Cylinder::isInside :324-329 (r^2 < R^2, no root) */
static __device__ __forceinline__ int shape_inside(int kind, const float* q, float x, float y, float z) {
	if (kind == 0) return x >= q[0] && y >= q[1] && z >= q[2] && x <= q[3] && y <= q[4] && z <= q[5];
	if (kind == 1) {
		const float a = (x - q[0]) / q[4], b = (y - q[1]) / q[5], c = (z - q[2]) / q[6];
		return (a * a + b * b + c * c) <= q[3] * q[3];
	}
	const float px = x - q[0], py = y - q[1], pz = z - q[2];
	const float zz = px * q[4] + py * q[5] + pz * q[6];
	if (fabsf(zz) > q[7]) return 0;
	const float r2 = (px * px + py * py + pz * pz) - zz * zz;
	return r2 < q[3] * q[3];
}

}  // namespace mf
