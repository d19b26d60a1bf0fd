// movingobs.hip -- moving obstacles and the obstacle coupling of the FLIP scenes (include/open/manta_hip_movingobs.h): bandwidth-bound
// stencil and element-wise kernels, one thread per cell (lanes along x) or per particle, one launch each.
// Reference: movingobs.cpp, particle.h:551-578, plugin/extforces.cpp:337-373, grid.cpp:306-319, 672-715, 930-985, fastmarch.cpp:303-375,
// plugin/advection.cpp:397-402, commonkernels.h:67-72.
#include "common.h"
#include "extrap_passes.h"
#include "scan.h"
#include "shape_inside.h"
#include "../../include/open/manta_hip_movingobs.h"

using namespace mf;

namespace {

constexpr int MF_SURFACE = 128;   // FlagGrid::TypeSurface

// ---- kn_set_wall_bcs2, extforces.cpp:339-368 (KERNEL(): every cell; a thread writes its own cell only) ----
__global__ void __launch_bounds__(BLOCK)
k_set_wall_bcs2(Dim d, const int32_t* __restrict__ flags, float* __restrict__ vel, const float* __restrict__ obvel) {
	CELL_IJK(d)
	const int64_t n = d.n;
	const int f = flags[idx];
	if (i > 0) {
		const int both = f | flags[idx - 1];
		if ((both & MF_FLUID) && (both & MF_OBSTACLE)) vel[idx] = obvel[idx];
	}
	if (j > 0) {
		const int both = f | flags[idx - d.Y];
		if ((both & MF_FLUID) && (both & MF_OBSTACLE)) vel[n + idx] = obvel[n + idx];
	}
	if (!d.is3d) {
		vel[2 * n + idx] = 0.f;
	} else if (k > 0) {
		const int both = f | flags[idx - d.Z];
		if ((both & MF_FLUID) && (both & MF_OBSTACLE)) vel[2 * n + idx] = obvel[2 * n + idx];
	}
}

// ---- knSetBoundaryMAC / knSetBoundaryMACNorm / kn_set_bound_MAC2, grid.cpp:672-710 ----
__global__ void __launch_bounds__(BLOCK) k_set_bound_mac(Dim d, float* __restrict__ vel, float vx, float vy, float vz, int w, int rule) {
	CELL_IJK(d)
	const int sx = d.sx, sy = d.sy, sz = d.sz;
	const bool z3 = d.is3d;
	bool bx, by, bz;
	if (rule == 0) {
		const bool zin = z3 && (k <= w - 1 || k >= sz - 1 - w);
		bx = i <= w || i >= sx - w || j <= w - 1 || j >= sy - 1 - w || zin;
		by = i <= w - 1 || i >= sx - 1 - w || j <= w || j >= sy - w || zin;
		bz = i <= w - 1 || i >= sx - 1 - w || j <= w - 1 || j >= sy - 1 - w || (z3 && (k <= w || k >= sz - w));
	} else if (rule == 1) {
		bx = i <= w || i >= sx - w;
		by = j <= w || j >= sy - w;
		bz = z3 && (k <= w || k >= sz - w);
	} else {
		const bool xin = i <= w || i >= sx - 1 - w, yin = j <= w || j >= sy - 1 - w, zin = z3 && (k <= w || k >= sz - 1 - w);
		bx = i <= w + 1 || i >= sx - 1 - w || yin || zin;
		by = xin || j <= w + 1 || j >= sy - 1 - w || zin;
		bz = xin || yin || (z3 && (k <= w + 1 || k >= sz - 1 - w));
	}
	if (bx) vel[idx] = vx;
	if (by) vel[d.n + idx] = vy;
	if (bz) vel[2 * d.n + idx] = vz;
}

// ---- FlagGrid::mark_surface, grid.cpp:930-972 ----
// is_boundary(p, bnd = 0), grid.h:447-458, of a cell inside the grid: the outermost layer
__device__ __forceinline__ bool on_boundary(const Dim& d, int i, int j, int k) {
	bool r = i <= 0 || i >= d.sx - 1 || j <= 0 || j >= d.sy - 1;
	if (d.is3d) r = r || k <= 0 || k >= d.sz - 1;
	return r;
}
// In place.  The reference's loop over the neighbours stops at the first one that is outside the grid, or that is not a boundary cell
// and not fluid; so the cell is marked iff such a neighbour exists, whatever the order.  Why in place is race-free: a thread stores to
// its own word only, and the store changes the TypeSurface bit alone; the other threads read that word for its TypeFluid bit, which is
// the same in every value the word holds during the launch.  The concurrent accesses to one word are relaxed atomics (a 32-bit load /
// store each, never torn), so the HIP memory model has no data race here, and whichever value a load returns, the bit it looks at is
// the one the launch started with.
__global__ void __launch_bounds__(BLOCK) k_mark_surface(Dim d, int32_t* flags) {
	CELL_IJK(d)
	const int f = __hip_atomic_load(flags + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	int out = f & ~MF_SURFACE;
	if (f & MF_FLUID) {
		bool mark = false;
		const int k0 = d.is3d ? -1 : 0, k1 = d.is3d ? 1 : 0;
		for (int dk = k0; dk <= k1 && !mark; dk++)
			for (int dj = -1; dj <= 1 && !mark; dj++)
				for (int di = -1; di <= 1; di++) {
					if (!di && !dj && !dk) continue;
					const int ii = i + di, jj = j + dj, kk = k + dk;
					if (!in_grid(d, ii, jj, kk)) {
						mark = true;
						break;
					}
					if (on_boundary(d, ii, jj, kk)) continue;
					const int g = __hip_atomic_load(flags + (idx + di + dj * d.Y + dk * d.Z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if (!(g & MF_FLUID)) {
						mark = true;
						break;
					}
				}
		if (mark) out |= MF_SURFACE;
	}
	if (out != f) __hip_atomic_store(flags + idx, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- FlagGrid::clear_obstacle, grid.cpp:974-984 ----
__global__ void __launch_bounds__(BLOCK) k_clear_obstacle(Dim d, int32_t* __restrict__ flags, int include_boundary) {
	CELL_IJK(d)
	if (!(flags[idx] & MF_OBSTACLE)) return;
	if (!include_boundary && on_boundary(d, i, j, k)) return;
	flags[idx] = MF_EMPTY;
}

// ---- knGridClampNorm, grid.cpp:306-312: `me[idx] *= val / n` is one fp32 quotient, then Vector3D::operator*=(S) ----
template <int NCOMP>
__global__ void __launch_bounds__(BLOCK) k_clamp_norm(int64_t n, float* __restrict__ data, float val) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	if (NCOMP == 1) {
		const float v = data[idx];
		const float nn = sqrtf(v * v);
		if (nn > val) data[idx] = v * (val / nn);
	} else {
		const float x = data[idx], y = data[n + idx], z = data[2 * n + idx];
		const float nn = sqrtf(x * x + y * y + z * z);
		if (nn > val) {
			const float s = val / nn;
			data[idx] = x * s;
			data[n + idx] = y * s;
			data[2 * n + idx] = z * s;
		}
	}
}

// ---- knResetPhiInObs, advection.cpp:397-401 ----
__global__ void __launch_bounds__(BLOCK) k_reset_phi_in_obs(int64_t n, const int32_t* __restrict__ flags, float* __restrict__ sdf) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	if ((flags[idx] & MF_OBSTACLE) && sdf[idx] < 0.f) sdf[idx] = (float)0.1;
}

// normalize(Vector3D<float>&), vectorbase.h:420-434: the two epsilon branches; `v *= 1./norm` multiplies by the double quotient rounded
// to fp32.  Returns the norm.
__device__ __forceinline__ float normalize3(float& x, float& y, float& z) {
	const float l = x * x + y * y + z * z;
	const float eps2 = 1e-6f * 1e-6f;
	if (fabs((double)l - 1.) < (double)eps2) return 1.f;
	if (l > eps2) {
		const float nrm = sqrtf(l);
		const float fac = (float)(1. / (double)nrm);
		x *= fac;
		y *= fac;
		z *= fac;
		return nrm;
	}
	x = y = z = 0.f;
	return 0.f;
}

// ---- knUnprojectNormalComp, fastmarch.cpp:303-332 (KERNEL(bnd = 1)) ----
__global__ void __launch_bounds__(BLOCK) k_unproject_normal(Dim d, float* __restrict__ vel, const float* __restrict__ phi, float maxDist) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	const float p = phi[idx];
	if (p > 0.f || p < -maxDist) return;
	// getNormal: the centre is clamped to [1, size-2] (the upper clamp first, as in the reference); kd = 0 on a 2-D grid
	int ci = i, cj = j, ck = k;
	if (ci > d.sx - 2) ci = d.sx - 2;
	if (ci < 1) ci = 1;
	if (cj > d.sy - 2) cj = d.sy - 2;
	if (cj < 1) cj = 1;
	if (d.is3d) {
		if (ck > d.sz - 2) ck = d.sz - 2;
		if (ck < 1) ck = 1;
	}
	const int64_t c = (int64_t)ci + d.Y * cj + d.Z * ck;
	float nx = phi[c + 1] - phi[c - 1], ny = phi[c + d.Y] - phi[c - d.Y];
	float nz = d.is3d ? phi[c + d.Z] - phi[c - d.Z] : phi[c] - phi[c];
	const int64_t n = d.n;
	const float vx = vel[idx], vy = vel[n + idx], vz = vel[2 * n + idx];
	if (nx * vx + ny * vy + nz * vz < 0.f) {
		normalize3(nx, ny, nz);
		const float l = nx * vx + ny * vy + nz * vz;
		vel[idx] = vx - nx * l;
		vel[n + idx] = vy - ny * l;
		vel[2 * n + idx] = vz - nz * l;
	}
}

// ---- MovingObstacle::moveLinear, movingobs.cpp:70-91 ----
struct MoveShapes {
	int n;
	int kind[MF_MOVINGOBS_MAX_SHAPES];
	ShapeParams P[MF_MOVINGOBS_MAX_SHAPES];
};
// the reset and the stamping of every shape in one pass: a later write of the reference's sequence wins, and they all write the same
__global__ void __launch_bounds__(BLOCK) k_move_flags(Dim d, int32_t* __restrict__ flags, int id, int emptyType, MoveShapes S) {
	CELL_IJK(d)
	const int f = flags[idx];
	int out = (f & id) ? emptyType : f;
	const float x = (float)i + 0.5f, y = (float)j + 0.5f, z = (float)k + 0.5f;
	for (int s = 0; s < S.n; s++)
		if (shape_inside(S.kind[s], S.P[s].q, x, y, z)) {
			out = MF_OBSTACLE | id;
			break;
		}
	if (out != f) flags[idx] = out;
}
// FOR_IJK_BND(flags, 1) over the NEW flags.  On a 2-D grid flags(i, j, k-1) is the cell itself (the reference's z stride is 0,
// grid.cpp:56), so vel.z is written wherever the cell carries the ID: that branch is written out, plane -1 is never indexed.
__global__ void __launch_bounds__(BLOCK) k_move_vel(Dim d, const int32_t* __restrict__ flags, float* __restrict__ vel, int id, float vx, float vy, float vz) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	const bool cur = (flags[idx] & id) != 0;
	if (cur || (flags[idx - 1] & id) != 0) vel[idx] = vx;
	if (cur || (flags[idx - d.Y] & id) != 0) vel[d.n + idx] = vy;
	if (d.is3d) {
		if (cur || (flags[idx - d.Z] & id) != 0) vel[2 * d.n + idx] = vz;
	} else if (cur) {
		vel[2 * d.n + idx] = vz;
	}
}

// ---- MovingObstacle::projectOutside, movingobs.cpp:44-50 ----
__global__ void __launch_bounds__(BLOCK) k_obstacle_sign(int64_t n, const int32_t* __restrict__ flags, float* __restrict__ phi) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	phi[idx] = (flags[idx] & MF_OBSTACLE) ? -0.5f : 0.5f;
}
// GradientOp, commonkernels.h:67-72: 0.5 * difference is exact in either precision
__global__ void __launch_bounds__(BLOCK) k_gradient(Dim d, const float* __restrict__ phi, float* __restrict__ grad) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	grad[idx] = 0.5f * (phi[idx + 1] - phi[idx - 1]);
	grad[d.n + idx] = 0.5f * (phi[idx + d.Y] - phi[idx - d.Y]);
	grad[2 * d.n + idx] = d.is3d ? 0.5f * (phi[idx + d.Z] - phi[idx - d.Z]) : 0.f;
}

// ---- KnProjectParticles, particle.h:552-572 ----
// gradient.isInBounds(p): toVec3i truncates; on a 2-D grid the z index must be 0 (grid.h:430-438)
__device__ __forceinline__ bool pos_in_grid(const Dim& d, float x, float y, float z) {
	const int i = (int)x, j = (int)y, k = (int)z;
	const bool r = i >= 0 && j >= 0 && i < d.sx && j < d.sy;
	return r && (d.is3d ? (k >= 0 && k < d.sz) : k == 0);
}
__global__ void __launch_bounds__(BLOCK)
k_project_count(Dim d, int64_t np, int64_t ps, const float* __restrict__ pos, const int32_t* __restrict__ pflag, int32_t* __restrict__ counts) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p > np) return;
	int c = 0;
	if (p < np && !(pflag[p] & MF_PDELETE)) c = pos_in_grid(d, pos[p], pos[ps + p], pos[2 * ps + p]) ? 4 : 3;
	counts[p] = c;   // counts[np] = 0: the scan leaves the total there
}
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__global__ void __launch_bounds__(BLOCK)
k_project_apply(Dim d, int64_t np, int64_t ps, float* __restrict__ pos, const int32_t* __restrict__ pflag, const float* __restrict__ grad,
                const int32_t* __restrict__ offsets, const float* __restrict__ reals) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= np) return;
	if (pflag[p] & MF_PDELETE) return;
	int64_t o = offsets[p];
	float x = pos[p], y = pos[ps + p], z = pos[2 * ps + p];
	if (pos_in_grid(d, x, y, z)) {
		float nx = interpol1(d, grad, x, y, z), ny = interpol1(d, grad + d.n, x, y, z), nz = interpol1(d, grad + 2 * d.n, x, y, z);
		const float dist = normalize3(nx, ny, nz);
		// `n * (-dist + jlen * (1 + rand.getReal()))`: 1 + r is int + float, an fp32 sum; jlen is a double, so the factor is fp64 and
		// each component's product is rounded once
		const double fac = (double)(-dist) + 0.1 * (double)(1.f + reals[o]);
		o++;
		x += (float)((double)nx * fac);
		y += (float)((double)ny * fac);
		z += (float)((double)nz * fac);
	}
	const float jx = (float)(0.1 * (double)reals[o]), jy = (float)(0.1 * (double)reals[o + 1]), jz = (float)(0.1 * (double)reals[o + 2]);
	pos[p] = clampf(x, 1.f + jx, (float)(d.sx - 1) - jx);
	pos[ps + p] = clampf(y, 1.f + jy, (float)(d.sy - 1) - jy);
	pos[2 * ps + p] = clampf(z, 1.f + jz, (float)(d.sz - 1) - jz);
}

}  // namespace

extern "C" {

int mf_movingobs_abi_version(void) { return MF_MOVINGOBS_ABI_VERSION; }

int mf_movingobs_set_wall_bcs2(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* obvel, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (vel == obvel) return fail("set_wall_bcs2: vel must not alias obvel");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_set_wall_bcs2, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, vel, obvel);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_movingobs_set_bound_mac(int sx, int sy, int sz, float* vel, float valueX, float valueY, float valueZ, int w, int rule, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (rule < 0 || rule > 2) return fail("mf_movingobs_set_bound_mac: unknown rule %d", rule);
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_set_bound_mac, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, vel, valueX, valueY, valueZ, w, rule);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_movingobs_mark_surface(int sx, int sy, int sz, int32_t* flags, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_mark_surface, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_movingobs_clear_obstacle(int sx, int sy, int sz, int32_t* flags, int include_boundary, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_clear_obstacle, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, include_boundary);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_movingobs_clamp_norm(int64_t n, int ncomp, float* data, float val, void* stream) {
	if (n < 0 || (ncomp != 1 && ncomp != 3)) return fail("mf_movingobs_clamp_norm: invalid size %lld / ncomp %d", (long long)n, ncomp);
	if (n == 0) return 0;
	if (ncomp == 1) hipLaunchKernelGGL(k_clamp_norm<1>, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, data, val);
	else hipLaunchKernelGGL(k_clamp_norm<3>, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, data, val);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_movingobs_reset_phi_in_obs(int64_t n, const int32_t* flags, float* sdf, void* stream) {
	if (n < 0) return fail("mf_movingobs_reset_phi_in_obs: negative size");
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_reset_phi_in_obs, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, flags, sdf);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_movingobs_extrapolate_mac_simple(int sx, int sy, int sz, const int32_t* flags, float* vel, int distance, int intoObs,
                                        const float* phiObs, int32_t* tmp, float* velTmp, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (!phiObs) return fail("mf_movingobs_extrapolate_mac_simple: phiObs is NULL (mf_extrapolate_mac_simple is the entry without it)");
	const Dim d = mkdim(sx, sy, sz);
	const hipStream_t st = (hipStream_t)stream;
	MF_TRY(extrap_component_passes(d, flags, vel, distance, intoObs, tmp, st));
	hipLaunchKernelGGL(k_unproject_normal, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, vel, phiObs, (float)distance);
	MF_LAUNCH_CHECK();
	return extrap_into_bnd(d, flags, vel, velTmp, st);
}

int mf_movingobs_move(int sx, int sy, int sz, int32_t* flags, float* vel, int id, int emptyType, int nshapes, const int32_t* kinds_host,
                      const float* params_host, float vx, float vy, float vz, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (nshapes < 0 || nshapes > MF_MOVINGOBS_MAX_SHAPES)
		return fail("MovingObstacle: %d shapes, at most %d are supported", nshapes, MF_MOVINGOBS_MAX_SHAPES);
	MoveShapes S;
	memset(&S, 0, sizeof(S));
	S.n = nshapes;
	for (int s = 0; s < nshapes; s++) {
		if (kinds_host[s] < 0 || kinds_host[s] > 2) return fail("MovingObstacle: unknown shape kind %d", (int)kinds_host[s]);
		S.kind[s] = kinds_host[s];
		for (int q = 0; q < 12; q++) S.P[s].q[q] = params_host[12 * s + q];
	}
	const Dim d = mkdim(sx, sy, sz);
	const hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_move_flags, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, flags, id, emptyType, S);
	hipLaunchKernelGGL(k_move_vel, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, flags, vel, id, vx, vy, vz);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_movingobs_obstacle_sign(int64_t n, const int32_t* flags, float* phi, void* stream) {
	if (n < 0) return fail("mf_movingobs_obstacle_sign: negative size");
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_obstacle_sign, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, flags, phi);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_movingobs_gradient(int sx, int sy, int sz, const float* phi, float* grad, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_gradient, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, phi, grad);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_movingobs_project_scratch(int64_t np, int64_t* bytes) {
	if (np < 0 || np >= ((int64_t)1 << 29)) return fail("projectOutside: invalid particle count %lld", (long long)np);
	size_t b = 0;
	MF_TRY(exclusive_sum32_bytes(np + 1, &b));
	*bytes = (int64_t)al256(b) + 256;
	return 0;
}

int mf_movingobs_project_count(int sx, int sy, int sz, int64_t np, int64_t pstride, const float* pos, const int32_t* pflag, int32_t* offsets,
                               void* tmp, int64_t tmp_bytes, int64_t* total_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	*total_host = 0;
	if (np < 0 || np >= ((int64_t)1 << 29)) return fail("projectOutside: invalid particle count %lld", (long long)np);   // 4 np < 2^31
	if (np == 0) return 0;
	size_t need = 0;
	MF_TRY(exclusive_sum32_bytes(np + 1, &need));
	if (!tmp || tmp_bytes < (int64_t)need) return fail("projectOutside: scratch of %lld bytes, %lld needed", (long long)tmp_bytes, (long long)need);
	const Dim d = mkdim(sx, sy, sz);
	const hipStream_t st = (hipStream_t)stream;
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	hipLaunchKernelGGL(k_project_count, dim3(nblk(np + 1)), dim3(BLOCK), 0, st, d, np, pstride, pos, pflag, offsets);
	MF_LAUNCH_CHECK();
	MF_TRY(exclusive_sum(tmp, (size_t)tmp_bytes, offsets, offsets, np + 1, st));
	int32_t total;
	MF_TRY(read_scalars(ws, offsets + np, sizeof(total), &total, st));
	*total_host = total;
	return 0;
}

int mf_movingobs_project_apply(int sx, int sy, int sz, int64_t np, int64_t pstride, float* pos, const int32_t* pflag, const float* grad,
                               const int32_t* offsets, const float* reals, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (np <= 0) return 0;
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_project_apply, dim3(nblk(np)), dim3(BLOCK), 0, (hipStream_t)stream, d, np, pstride, pos, pflag, grad, offsets, reals);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
