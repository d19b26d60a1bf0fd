// glue.hip -- the single-sweep kernels that sit between advection and the pressure solve in every smoke /
// FLIP scene, so that a step never leaves the device.  Reference: source/plugin/extforces.cpp.
#include "common.h"
#include "extrap_passes.h"

using namespace mf;

// KnSetWallBcs, extforces.cpp:187-237 (KERNEL(): every cell; each thread writes only its own cell)
__global__ void __launch_bounds__(BLOCK)
k_set_wall_bcs(Dim d, const int32_t* __restrict__ flags, float* __restrict__ vel, const float* __restrict__ obvel) {
	CELL_IJK(d)
	const int64_t n = d.n, Y = d.Y, Z = d.Z;
	const int f = flags[idx];
	const bool curFluid = f & MF_FLUID, curObs = f & MF_OBSTACLE;
	if (!curFluid && !curObs) return;
	float bx = 0.f, by = 0.f, bz = 0.f;
	if (obvel) {
		bx = obvel[idx];
		by = obvel[n + idx];
		if (d.is3d) bz = obvel[2 * n + idx];
	}
	float vx = vel[idx], vy = vel[n + idx], vz = vel[2 * n + idx];
	const int fxm = i > 0 ? flags[idx - 1] : 0, fym = j > 0 ? flags[idx - Y] : 0, fzm = (d.is3d && k > 0) ? flags[idx - Z] : 0;
	if (i > 0 && (fxm & MF_OBSTACLE)) vx = bx;
	if (i > 0 && curObs && (fxm & MF_FLUID)) vx = bx;
	if (j > 0 && (fym & MF_OBSTACLE)) vy = by;
	if (j > 0 && curObs && (fym & MF_FLUID)) vy = by;
	if (!d.is3d) {
		vz = 0.f;
	} else {
		if (k > 0 && (fzm & MF_OBSTACLE)) vz = bz;
		if (k > 0 && curObs && (fzm & MF_FLUID)) vz = bz;
	}
	if (curFluid) {
		if ((i > 0 && (fxm & MF_STICK)) || (i < d.sx - 1 && (flags[idx + 1] & MF_STICK))) vy = vz = 0.f;
		if ((j > 0 && (fym & MF_STICK)) || (j < d.sy - 1 && (flags[idx + Y] & MF_STICK))) vx = vz = 0.f;
		if (d.is3d && ((k > 0 && (fzm & MF_STICK)) || (k < d.sz - 1 && (flags[idx + Z] & MF_STICK)))) vx = vy = 0.f;
	}
	vel[idx] = vx;
	vel[n + idx] = vy;
	vel[2 * n + idx] = vz;
}

// KnAddBuoyancy, extforces.cpp:73-81: `vel += (0.5*strength) * (f0 + f1)` is an fp64 compound assignment
__global__ void __launch_bounds__(BLOCK)
k_add_buoyancy(Dim d, const int32_t* __restrict__ flags, const float* __restrict__ fac, float* __restrict__ vel, float fx, float fy, float fz) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	if (!(flags[idx] & MF_FLUID)) return;
	const int64_t n = d.n, Y = d.Y, Z = d.Z;
	const float f0 = fac[idx];
	if (flags[idx - 1] & MF_FLUID) vel[idx] = (float)((double)vel[idx] + (0.5 * (double)fx) * (double)(f0 + fac[idx - 1]));
	if (flags[idx - Y] & MF_FLUID) vel[n + idx] = (float)((double)vel[n + idx] + (0.5 * (double)fy) * (double)(f0 + fac[idx - Y]));
	if (d.is3d && (flags[idx - Z] & MF_FLUID))
		vel[2 * n + idx] = (float)((double)vel[2 * n + idx] + (0.5 * (double)fz) * (double)(f0 + fac[idx - Z]));
}

// KnApplyForce, extforces.cpp:46-60
__global__ void __launch_bounds__(BLOCK)
k_apply_force(Dim d, const int32_t* __restrict__ flags, float* __restrict__ vel, float fx, float fy, float fz,
              const float* __restrict__ exclude, int additive) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	const int64_t n = d.n, Y = d.Y, Z = d.Z;
	const bool curFluid = flags[idx] & MF_FLUID, curEmpty = flags[idx] & MF_EMPTY;
	if (!curFluid && !curEmpty) return;
	if (exclude && (exclude[idx] < 0.f)) return;
	const int fxm = flags[idx - 1], fym = flags[idx - Y];
	if ((fxm & MF_FLUID) || (curFluid && (fxm & MF_EMPTY))) vel[idx] = additive ? vel[idx] + fx : fx;
	if ((fym & MF_FLUID) || (curFluid && (fym & MF_EMPTY))) vel[n + idx] = additive ? vel[n + idx] + fy : fy;
	if (d.is3d) {
		const int fzm = flags[idx - Z];
		if ((fzm & MF_FLUID) || (curFluid && (fzm & MF_EMPTY))) vel[2 * n + idx] = additive ? vel[2 * n + idx] + fz : fz;
	}
}

// ---- FLIP glue ---------------------------------------------------------------------------------
// the component passes and the into-boundary copy of extrapolateMACSimple: extrap_passes.h (shared with movingobs.hip)
// extrapolateMACFromWeight, fastmarch.cpp:378-430
__global__ void __launch_bounds__(BLOCK) k_weight_reset(Dim d, float* __restrict__ wc) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	if (wc[idx] > 0.f) wc[idx] = 1.0f;
}
__global__ void __launch_bounds__(BLOCK)
k_extrap_weight(Dim d, float* __restrict__ velc, float* __restrict__ wc, int dd) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	if (wc[idx] != 0.f) return;
	const int64_t nb[6] = {1, -1, d.Y, -d.Y, d.Z, -d.Z};
	const int nn = d.is3d ? 6 : 4;
	int nbs = 0;
	float avg = 0.f;
	const float fd = (float)dd;
	for (int n = 0; n < nn; n++)
		if (wc[idx + nb[n]] == fd) {
			avg += velc[idx + nb[n]];
			nbs++;
		}
	if (nbs > 0) {
		wc[idx] = (float)(dd + 1);
		velc[idx] = avg / (float)nbs;
	}
}
// markFluidCells, flip.cpp:142-188
__global__ void __launch_bounds__(BLOCK) k_clear_fluid_flags(Dim d, int32_t* __restrict__ flags) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= d.n) return;
	const int f = flags[idx];
	if (f & MF_FLUID) flags[idx] = (f | MF_EMPTY) & ~MF_FLUID;
}
__global__ void __launch_bounds__(BLOCK)
k_mark_fluid(Dim d, int32_t* __restrict__ flags, int64_t np, int64_t ps, const float* __restrict__ pos,
             const int32_t* __restrict__ pflag, const int32_t* __restrict__ ptype, int exclude) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= np) return;
	if ((pflag[p] & MF_PDELETE) || (ptype && (ptype[p] & exclude))) return;
	const int i = (int)pos[p], j = (int)pos[ps + p];   // toVec3i truncation
	const int k = (int)pos[2 * ps + p] - d.zoff;       // plane inside the slab window (global coordinates; identity without one)
	if (i < 0 || j < 0 || k < 0 || i >= d.sx || j >= d.sy || k >= d.sz) return;
	const int64_t idx = (int64_t)i + d.Y * j + d.Z * k;
	const int f = flags[idx];
	// every particle of a cell writes the same value, so concurrent marking is order independent
	if (f & MF_EMPTY) flags[idx] = (f | MF_FLUID) & ~MF_EMPTY;
}
// knSetNbObstacle, flip.cpp:149-164
__global__ void __launch_bounds__(BLOCK)
k_set_nb_obstacle(Dim d, int32_t* __restrict__ nflags, const int32_t* __restrict__ flags, const float* __restrict__ phiObs) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	if (phiObs[idx] > 0.f) return;
	if (!(flags[idx] & MF_EMPTY)) return;
	bool set = false;
	if ((flags[idx - 1] & MF_FLUID) && (phiObs[idx + 1] <= 0.f)) set = true;
	if ((flags[idx + 1] & MF_FLUID) && (phiObs[idx - 1] <= 0.f)) set = true;
	if ((flags[idx - d.Y] & MF_FLUID) && (phiObs[idx + d.Y] <= 0.f)) set = true;
	if ((flags[idx + d.Y] & MF_FLUID) && (phiObs[idx - d.Y] <= 0.f)) set = true;
	if (d.is3d) {
		if ((flags[idx - d.Z] & MF_FLUID) && (phiObs[idx + d.Z] <= 0.f)) set = true;
		if ((flags[idx + d.Z] & MF_FLUID) && (phiObs[idx - d.Z] <= 0.f)) set = true;
	}
	if (set) nflags[idx] = (flags[idx] | MF_FLUID) & ~MF_EMPTY;
}

extern "C" {
int mf_extrapolate_mac_simple(int sx, int sy, int sz, const int32_t* flags, float* vel, int distance, int intoObs,
                              int32_t* tmp, float* velTmp, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	MF_TRY(extrap_component_passes(d, flags, vel, distance, intoObs, tmp, st));
	return extrap_into_bnd(d, flags, vel, velTmp, st);
}
int mf_extrapolate_mac_from_weight(int sx, int sy, int sz, float* vel, float* weight, int distance, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	const int dim = d.is3d ? 3 : 2;
	for (int c = 0; c < dim; c++) {
		hipLaunchKernelGGL(k_weight_reset, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, weight + c * d.n);
		for (int dd = 1; dd < 1 + distance; dd++)
			hipLaunchKernelGGL(k_extrap_weight, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, vel + c * d.n, weight + c * d.n, dd);
	}
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_mark_fluid_cells(int sx, int sy, int sz, int32_t* flags, int64_t np, int64_t ps, const float* pos, const int32_t* pflag,
                        const int32_t* ptype, int exclude, const float* phiObs, int32_t* ftmp, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_clear_fluid_flags, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, flags);
	if (np > 0)
		hipLaunchKernelGGL(k_mark_fluid, dim3((unsigned)((np + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, d, flags, np, ps, pos, pflag, ptype, exclude);
	if (phiObs) {
		// FlagGrid tmp(flags); knSetNbObstacle(tmp, flags, phiObs); flags.swap(tmp)
		MF_HIP(hipMemcpyAsync(ftmp, flags, sizeof(int32_t) * d.n, hipMemcpyDeviceToDevice, st));
		hipLaunchKernelGGL(k_set_nb_obstacle, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, ftmp, flags, phiObs);
		MF_HIP(hipMemcpyAsync(flags, ftmp, sizeof(int32_t) * d.n, hipMemcpyDeviceToDevice, st));
	}
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_set_wall_bcs(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* obvel, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_set_wall_bcs, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, vel, obvel);
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_add_buoyancy(int sx, int sy, int sz, const int32_t* flags, const float* density, float* vel, float fx, float fy, float fz, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_add_buoyancy, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, density, vel, fx, fy, fz);
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_apply_force(int sx, int sy, int sz, const int32_t* flags, float* vel, float fx, float fy, float fz, const float* exclude,
                   int additive, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_apply_force, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, vel, fx, fy, fz, exclude, additive);
	MF_LAUNCH_CHECK();
	return 0;
}
}  // extern "C"
