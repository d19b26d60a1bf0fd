// obstacles.hip -- fill-fraction obstacle boundaries (include/manta_hip_obstacles.h): updateFractions, setObstacleFlags,
// setWallBcs in fraction mode, setInflowBcs.  Reference: source/plugin/initplugins.cpp, source/plugin/extforces.cpp.
// addNoise lives in noise.hip beside the noise evaluation it shares with densityInflow.
#include "common.h"
#include "../../include/manta_hip_obstacles.h"

using namespace mf;

namespace {

constexpr int OPENISH = MF_INFLOW | MF_OUTFLOW | MF_OPEN;

// the cells a KERNEL(bnd=b) visits (KernelBase::KernelBase, kernel.cpp:21-30, and the generated run(): the k loop runs
// [minZ, maxZ) when maxZ > 1, else the single plane k = 0)
__device__ __forceinline__ bool in_kernel_range(const Dim& d, int b, int i, int j, int k) {
	if (i < b || i >= d.sx - b || j < b || j >= d.sy - b) return false;
	const int maxZ = d.is3d ? d.sz - b : 1, minZ = d.is3d ? b : 0;
	return maxZ > 1 ? (k >= minZ && k < maxZ) : k == 0;
}

// calcFraction, initplugins.cpp:356-371 (Real = float; the 1e-04 test and "1. - phi1/denom" are evaluated in double)
__device__ __forceinline__ float calc_fraction(float phi1, float phi2, float thr) {
	if (phi1 > 0.f && phi2 > 0.f) return 1.f;
	if (phi1 < 0.f && phi2 < 0.f) return 0.f;
	if (phi2 < phi1) {
		const float t = phi1;
		phi1 = phi2;
		phi2 = t;
	}
	const float denom = phi1 - phi2;
	if ((double)denom > -1e-04) return 0.5f;
	float frac = (float)(1. - (double)(phi1 / denom));
	if (frac < thr) frac = 0.f;
	return frac < 1.f ? frac : 1.f;   // std::min(Real(1), frac)
}

// KnUpdateFractions (bnd=1) after fractions.setConst(0), initplugins.cpp:373-440, as a gather: every face is written by the thread
// of its own cell.  A cell inside the bnd=1 range ends with its own result (its own calcFraction and "min" rules run after every
// earlier "max" write into it in the serial sweep); a cell outside keeps 0 unless the "max" rule of its -x, -y or -z neighbour
// (a cell inside the range, not in the obstacle) set it to 1.
__global__ void __launch_bounds__(BLOCK)
k_update_fractions(Dim d, const int32_t* __restrict__ flags, const float* __restrict__ phi, float* __restrict__ fr, int w, float thr) {
	CELL_IJK(d)
	const int64_t n = d.n, Y = d.Y, Z = d.Z;
	float fx = 0.f, fy = 0.f, fz = 0.f;
	bool one = false;
	if (in_kernel_range(d, 1, i, j, k)) {
		const float p = phi[idx];
		fx = calc_fraction(p, phi[idx - 1], thr);
		fy = calc_fraction(p, phi[idx - Y], thr);
		if (d.is3d) fz = calc_fraction(p, phi[idx - Z], thr);
		if (!(p < 0.f)) {
			if (i <= w + 1 && (flags[idx - 1] & OPENISH)) one = true;                // min x
			if (j <= w + 1 && (flags[idx - Y] & OPENISH)) one = true;                // min y
			if (d.is3d && k <= w + 1 && (flags[idx - Z] & OPENISH)) one = true;      // min z
		}
	} else if (flags[idx] & OPENISH) {
		if (in_kernel_range(d, 1, i - 1, j, k) && !(phi[idx - 1] < 0.f) && i - 1 >= d.sx - w - 2) one = true;   // max x of (i-1)
		if (in_kernel_range(d, 1, i, j - 1, k) && !(phi[idx - Y] < 0.f) && j - 1 >= d.sy - w - 2) one = true;   // max y of (j-1)
		if (d.is3d && in_kernel_range(d, 1, i, j, k - 1) && !(phi[idx - Z] < 0.f) && j >= d.sz - w - 2) one = true;   // max z: j, as in the reference
	}
	if (one) {
		fx = fy = 1.f;
		if (d.is3d) fz = 1.f;
	}
	fr[idx] = fx;
	fr[n + idx] = fy;
	fr[2 * n + idx] = fz;
}

// KnUpdateFlagsObs, initplugins.cpp:442-468
__global__ void __launch_bounds__(BLOCK)
k_set_obstacle_flags(Dim d, int32_t* __restrict__ flags, const float* __restrict__ phi, const float* __restrict__ fr,
                     const float* __restrict__ phiOut, const float* __restrict__ phiIn, int b) {
	CELL_IJK(d)
	if (!in_kernel_range(d, b, i, j, k)) return;
	const int64_t n = d.n, Y = d.Y, Z = d.Z;
	bool isObs = false;
	if (fr) {
		float f = 0.f;
		f += fr[idx];
		f += fr[idx + 1];
		f += fr[n + idx];
		f += fr[n + idx + Y];
		if (d.is3d) {
			f += fr[2 * n + idx];
			f += fr[2 * n + idx + Z];
		}
		if (f == 0.f) isObs = true;
	} else {
		if (phi[idx] < 0.f) isObs = true;
	}
	const bool isOutflow = phiOut && phiOut[idx] < 0.f;
	const bool isInflow = phiIn && phiIn[idx] < 0.f;
	int v = MF_EMPTY;
	if (isObs) v = MF_OBSTACLE;
	else if (isInflow) v = MF_FLUID | MF_INFLOW;
	else if (isOutflow) v = MF_EMPTY | MF_OUTFLOW;
	flags[idx] = v;
}

// normalize(Vec3&), util/vectorbase.h:421-433, S = float: |v|^2 in float, the "== 1" test in double, v *= (float)(1./norm)
__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
	const float l = x * x + y * y + z * z;
	const float eps2 = 1e-6f * 1e-6f;
	if (fabs((double)l - 1.) < (double)eps2) {
	} else if (l > eps2) {
		const float norm = sqrtf(l);
		const float s = (float)(1. / (double)norm);
		x *= s;
		y *= s;
		z *= s;
	} else {
		x = y = z = 0.f;
	}
}
// (a + b) * .5 of the reference: float sum, exact halving
__device__ __forceinline__ float avg2(float a, float b) { return (float)((double)(a + b) * .5); }
// velMAC.c - dot(dphi, velMAC) * dphi.c (vectorbase.h dot: x*x + y*y + z*z, left to right)
__device__ __forceinline__ float unproject(float dx, float dy, float dz, float vx, float vy, float vz, float vc, float dc) {
	const float dt = dx * vx + dy * vy + dz * vz;
	return vc - dt * dc;
}

// KnSetWallBcsFrac, extforces.cpp:240-324, first half: every cell with isInBounds(p, 1) that is fluid or obstacle computes the new
// value of each of its faces the reference rewrites, reading only the original velocities, and stores it at the face's own slot of
// `vals`; one wave ballot per component records which faces of the wave's 64 cells carry a new value.  Nothing of vel is written.
__global__ void __launch_bounds__(BLOCK)
k_wall_bcs_frac_collect(Dim d, const int32_t* __restrict__ flags, const float* __restrict__ vel, const float* __restrict__ phi,
                        float* __restrict__ vals, unsigned long long* __restrict__ mask) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	const int64_t n = d.n, Y = d.Y, Z = d.Z;
	bool cx = false, cy = false, cz = false;
	if (idx < n) {
		const unsigned t = (unsigned)idx / (unsigned)d.sx;
		const int i = (int)((unsigned)idx - t * (unsigned)d.sx), j = (int)(t % (unsigned)d.sy), k = (int)(t / (unsigned)d.sy);
		const int f = flags[idx];
		const bool curObs = f & MF_OBSTACLE;
		const bool inb = i >= 1 && j >= 1 && i < d.sx - 1 && j < d.sy - 1 && (d.is3d ? (k >= 1 && k < d.sz - 1) : k == 0);
		if ((f & (MF_FLUID | MF_OBSTACLE)) && inb) {
			cx = curObs || (flags[idx - 1] & MF_OBSTACLE);
			cy = curObs || (flags[idx - Y] & MF_OBSTACLE);
			cz = d.is3d && (curObs || (flags[idx - Z] & MF_OBSTACLE));
			const float p0 = phi[idx];
			if (cx) {
				const float pm = phi[idx - 1];
				const float tmp1 = avg2(p0, pm);
				float tmp2 = avg2(phi[idx + Y], phi[idx - 1 + Y]);
				float phi1 = avg2(tmp1, tmp2);
				tmp2 = avg2(phi[idx - Y], phi[idx - 1 - Y]);
				float phi2 = avg2(tmp1, tmp2);
				float dx = p0 - pm, dy = phi1 - phi2, dz = 0.f;
				if (d.is3d) {
					tmp2 = avg2(phi[idx + Z], phi[idx - 1 + Z]);
					phi1 = avg2(tmp1, tmp2);
					tmp2 = avg2(phi[idx - Z], phi[idx - 1 - Z]);
					phi2 = avg2(tmp1, tmp2);
					dz = phi1 - phi2;
				}
				normalize3(dx, dy, dz);
				float vx, vy, vz;
				get_at_mac_x(d, vel, idx, vx, vy, vz);
				vals[idx] = unproject(dx, dy, dz, vx, vy, vz, vx, dx);
			}
			if (cy) {
				const float pm = phi[idx - Y];
				const float tmp1 = avg2(p0, pm);
				float tmp2 = avg2(phi[idx + 1], phi[idx + 1 - Y]);
				float phi1 = avg2(tmp1, tmp2);
				tmp2 = avg2(phi[idx - 1], phi[idx - 1 - Y]);
				float phi2 = avg2(tmp1, tmp2);
				float dx = phi1 - phi2, dy = p0 - pm, dz = 0.f;
				if (d.is3d) {
					tmp2 = avg2(phi[idx + Z], phi[idx - Y + Z]);
					phi1 = avg2(tmp1, tmp2);
					tmp2 = avg2(phi[idx - Z], phi[idx - Y - Z]);
					phi2 = avg2(tmp1, tmp2);
					dz = phi1 - phi2;
				}
				normalize3(dx, dy, dz);
				float vx, vy, vz;
				get_at_mac_y(d, vel, idx, vx, vy, vz);
				vals[n + idx] = unproject(dx, dy, dz, vx, vy, vz, vy, dy);
			}
			if (cz) {
				const float pm = phi[idx - Z];
				const float tmp1 = avg2(p0, pm);
				float tmp2 = avg2(phi[idx + 1], phi[idx + 1 - Z]);
				float phi1 = avg2(tmp1, tmp2);
				tmp2 = avg2(phi[idx - 1], phi[idx - 1 - Z]);
				float phi2 = avg2(tmp1, tmp2);
				const float dx0 = phi1 - phi2;
				tmp2 = avg2(phi[idx + Y], phi[idx + Y - Z]);
				phi1 = avg2(tmp1, tmp2);
				tmp2 = avg2(phi[idx - Y], phi[idx - Y - Z]);
				phi2 = avg2(tmp1, tmp2);
				float dx = dx0, dy = phi1 - phi2, dz = p0 - pm;
				normalize3(dx, dy, dz);
				float vx, vy, vz;
				get_at_mac_z(d, vel, idx, vx, vy, vz);
				vals[2 * n + idx] = unproject(dx, dy, dz, vx, vy, vz, vz, dz);
			}
		}
	}
	// every lane of the wave reaches the ballots (blockDim is a multiple of 64, blocks start on a multiple of 64 cells)
	const unsigned long long bx = __ballot(cx), by = __ballot(cy), bz = __ballot(cz);
	const int64_t wv = idx >> 6;
	const int64_t nw = (n + 63) >> 6;
	if ((threadIdx.x & 63) == 0 && wv < nw) {
		mask[wv] = bx;
		mask[nw + wv] = by;
		mask[2 * nw + wv] = bz;
	}
}
// second half (the swap): the marked faces take their new values
__global__ void __launch_bounds__(BLOCK)
k_wall_bcs_frac_apply(Dim d, float* __restrict__ vel, const float* __restrict__ vals, const unsigned long long* __restrict__ mask) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= d.n) return;
	const int64_t n = d.n, nw = (n + 63) >> 6, wv = idx >> 6;
	const unsigned long long bit = 1ull << (idx & 63);
	if (mask[wv] & bit) vel[idx] = vals[idx];
	if (mask[nw + wv] & bit) vel[n + idx] = vals[n + idx];
	if (mask[2 * nw + wv] & bit) vel[2 * n + idx] = vals[2 * n + idx];
}

// KnSetInflow, extforces.cpp:163-168, for every side of `sides` at once (they all store the same value)
__global__ void __launch_bounds__(BLOCK)
k_set_inflow(Dim d, float* __restrict__ vel, int sides, float vx, float vy, float vz) {
	CELL_IJK(d)
	const int p[3] = {i, j, k}, s[3] = {d.sx, d.sy, d.sz};
	bool hit = false;
	for (int c = 0; c < 3; c++) {
		if ((sides >> (2 * c)) & 1) hit |= p[c] == 0 || p[c] == 1;
		if ((sides >> (2 * c + 1)) & 1) hit |= p[c] == s[c] - 1;
	}
	if (!hit) return;
	vel[idx] = vx;
	vel[d.n + idx] = vy;
	vel[2 * d.n + idx] = vz;
}

int64_t wall_frac_words(int64_t n) { return 6 * ((n + 63) >> 6) + 3 * n; }

}  // namespace

extern "C" {

int mf_obstacles_abi_version(void) { return MF_OBSTACLES_ABI_VERSION; }

int mf_update_fractions(int sx, int sy, int sz, const int32_t* flags, const float* phiObs, float* fractions, int boundaryWidth,
                        float fracThreshold, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (sz == 2) return fail("mf_update_fractions: a 3-D grid needs sz >= 3");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_update_fractions, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, phiObs, fractions,
	                   boundaryWidth, fracThreshold);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_set_obstacle_flags(int sx, int sy, int sz, int32_t* flags, const float* phiObs, const float* fractions, const float* phiOut,
                          const float* phiIn, int boundaryWidth, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (boundaryWidth < 0 || (fractions && boundaryWidth < 1))
		return fail("setObstacleFlags: boundaryWidth %d %s", boundaryWidth,
		            boundaryWidth < 0 ? "is negative" : "with fractions reads faces outside the grid (needs >= 1)");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_set_obstacle_flags, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, phiObs, fractions, phiOut,
	                   phiIn, boundaryWidth);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_set_wall_bcs_frac_scratch_words(int sx, int sy, int sz, int64_t* words) {
	MF_TRY(check_dim(sx, sy, sz));
	*words = wall_frac_words((int64_t)sx * sy * sz);
	return 0;
}

int mf_set_wall_bcs_frac(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* phiObs, uint32_t* scratch,
                         int64_t scratchWords, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	if (scratchWords < wall_frac_words(d.n))
		return fail("mf_set_wall_bcs_frac: scratch of %lld words, needs %lld", (long long)scratchWords, (long long)wall_frac_words(d.n));
	if (((uintptr_t)scratch & 7) != 0) return fail("mf_set_wall_bcs_frac: scratch must be 8-byte aligned");
	unsigned long long* mask = (unsigned long long*)scratch;
	float* vals = (float*)(scratch + 6 * ((d.n + 63) >> 6));
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_wall_bcs_frac_collect, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, flags, vel, phiObs, vals, mask);
	hipLaunchKernelGGL(k_wall_bcs_frac_apply, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, vel, vals, mask);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_set_inflow_bcs(int sx, int sy, int sz, float* vel, int sides, float vx, float vy, float vz, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (sides & ~63) return fail("mf_set_inflow_bcs: unknown side bits 0x%x", sides);
	const Dim d = mkdim(sx, sy, sz);
	if (sides == 0) return 0;
	hipLaunchKernelGGL(k_set_inflow, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, vel, sides, vx, vy, vz);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
