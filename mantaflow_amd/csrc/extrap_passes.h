// extrap_passes.h -- the pieces of extrapolateMACSimple (fastmarch.cpp:231-300, 337-375) that its two entries share: glue.hip's
// mf_extrapolate_mac_simple and movingobs.hip's mf_movingobs_extrapolate_mac_simple, which runs knUnprojectNormalComp between the
// component passes and the into-boundary copy.  One definition each; the kernels are internal to each translation unit.
#pragma once
#include "common.h"

namespace mf {

// marking pass of extrapolateMACSimple (serial FOR_IJK_BND in the reference, fastmarch.cpp:344-356): tmp = 1 where the
// face belongs to the fluid
static __global__ void __launch_bounds__(BLOCK)
k_extrap_mark(Dim d, const int32_t* __restrict__ flags, int32_t* __restrict__ tmp, int c, int intoObs) {
	CELL_IJK(d)
	int v = 0;
	if (INTERIOR(d)) {
		const int64_t o = c == 0 ? 1 : (c == 1 ? d.Y : d.Z);
		const int f0 = flags[idx], f1 = flags[idx - o];
		bool mark = (f0 & MF_FLUID) || (f1 & MF_FLUID);
		if (intoObs) mark = mark && !(f0 & MF_OBSTACLE) && !(f1 & MF_OBSTACLE);
		v = mark ? 1 : 0;
	}
	tmp[idx] = v;
}
// knExtrapolateMACSimple, fastmarch.cpp:231-259.  In place like the reference: a pass only reads cells whose marker
// equals d and only writes cells whose marker is 0 (to d+1), so the result does not depend on the thread order.
static __global__ void __launch_bounds__(BLOCK)
k_extrap_simple(Dim d, float* __restrict__ velc, int32_t* __restrict__ tmp, int dd) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	if (tmp[idx] != 0) return;
	const int64_t nb[6] = {1, -1, d.Y, -d.Y, d.Z, -d.Z};
	const int nn = d.is3d ? 6 : 4;
	int nbs = 0;
	float avg = 0.f;
	for (int n = 0; n < nn; n++)
		if (tmp[idx + nb[n]] == dd) {
			avg += velc[idx + nb[n]];
			nbs++;
		}
	if (nbs > 0) {
		tmp[idx] = dd + 1;
		velc[idx] = avg / (float)nbs;
	}
}
// The same pass with four consecutive cells per thread (3-D): the markers of the quad and of its +-Y / +-Z neighbour quads come as
// 16-byte loads (the +-Y ones from 4-byte aligned addresses when the row length is not a multiple of 4), 7 load instructions per 4 cells
// instead of 28 -- nearly every cell of a liquid scene only ever reads markers (12 passes per extrapolateMACSimple call).  Neighbour
// order and arithmetic per cell as above.
struct __attribute__((packed, aligned(4))) I4u {
	int x, y, z, w;
};
static __global__ void __launch_bounds__(BLOCK)
k_extrap_simple4(Dim d, float* __restrict__ velc, int32_t* __restrict__ tmp, int dd) {
	const int64_t idx0 = 4 * (blockIdx.x * (int64_t)BLOCK + threadIdx.x);
	if (idx0 + 3 >= d.n) {
		// (the last, partial quad of a grid whose cell count is not a multiple of 4: border cells of the last plane -- never interior)
		return;
	}
	const int4 m4 = *(const int4*)(tmp + idx0);
	const int m[4] = {m4.x, m4.y, m4.z, m4.w};
	if (m[0] != 0 && m[1] != 0 && m[2] != 0 && m[3] != 0) return;
	const int64_t Y = d.Y, Z = d.Z;
	int i = (int)(idx0 % d.sx), j = (int)((idx0 / d.sx) % d.sy), k = (int)(idx0 / ((int64_t)d.sx * d.sy));
	// neighbour markers; a quad that would reach outside the grid belongs to border cells only, which do nothing
	const int ml = idx0 > 0 ? tmp[idx0 - 1] : 0, mr = idx0 + 4 < d.n ? tmp[idx0 + 4] : 0;
	I4u yp = {0, 0, 0, 0}, ym = {0, 0, 0, 0};
	int4 zp = make_int4(0, 0, 0, 0), zm = make_int4(0, 0, 0, 0);
	if (idx0 + Y + 3 < d.n) yp = *(const I4u*)(tmp + idx0 + Y);
	if (idx0 - Y >= 0) ym = *(const I4u*)(tmp + idx0 - Y);
	const bool zal = (Z & 3) == 0;
	if (idx0 + Z + 3 < d.n) {
		if (zal) zp = *(const int4*)(tmp + idx0 + Z);
		else {
			const I4u t = *(const I4u*)(tmp + idx0 + Z);
			zp = make_int4(t.x, t.y, t.z, t.w);
		}
	}
	if (idx0 - Z >= 0) {
		if (zal) zm = *(const int4*)(tmp + idx0 - Z);
		else {
			const I4u t = *(const I4u*)(tmp + idx0 - Z);
			zm = make_int4(t.x, t.y, t.z, t.w);
		}
	}
	const int nxp[4] = {m[1], m[2], m[3], mr}, nxm[4] = {ml, m[0], m[1], m[2]};
	const int nyp[4] = {yp.x, yp.y, yp.z, yp.w}, nym[4] = {ym.x, ym.y, ym.z, ym.w};
	const int nzp[4] = {zp.x, zp.y, zp.z, zp.w}, nzm[4] = {zm.x, zm.y, zm.z, zm.w};
#pragma unroll
	for (int c = 0; c < 4; c++) {
		const int64_t idx = idx0 + c;
		const bool interior = i >= 1 && i < d.sx - 1 && j >= 1 && j < d.sy - 1 && k >= 1 && k < d.sz - 1;
		if (interior && m[c] == 0) {
			int nbs = 0;
			float avg = 0.f;
			if (nxp[c] == dd) { avg += velc[idx + 1]; nbs++; }
			if (nxm[c] == dd) { avg += velc[idx - 1]; nbs++; }
			if (nyp[c] == dd) { avg += velc[idx + Y]; nbs++; }
			if (nym[c] == dd) { avg += velc[idx - Y]; nbs++; }
			if (nzp[c] == dd) { avg += velc[idx + Z]; nbs++; }
			if (nzm[c] == dd) { avg += velc[idx - Z]; nbs++; }
			if (nbs > 0) {
				tmp[idx] = dd + 1;
				velc[idx] = avg / (float)nbs;
			}
		}
		// next cell of the quad
		if (++i == d.sx) {
			i = 0;
			if (++j == d.sy) {
				j = 0;
				k++;
			}
		}
	}
}
// knExtrapolateIntoBnd, fastmarch.cpp:261-300 (bnd = 0: every cell; only border cells change)
static __global__ void __launch_bounds__(BLOCK)
k_extrap_into_bnd(Dim d, const int32_t* __restrict__ flags, float* __restrict__ vel, const float* __restrict__ velTmp) {
	CELL_IJK(d)
	const int64_t n = d.n;
	int cnt = 0;
	float v0 = 0.f, v1 = 0.f, v2 = 0.f;
	const bool isObs = flags[idx] & MF_OBSTACLE;
#define TAKE(q, comp, cond)                                            \
	{                                                                  \
		v0 = velTmp[q];                                                \
		v1 = velTmp[n + (q)];                                          \
		v2 = velTmp[2 * n + (q)];                                      \
		if (isObs && (cond)) { if (comp == 0) v0 = 0.f; else if (comp == 1) v1 = 0.f; else v2 = 0.f; } \
		cnt++;                                                         \
	}
	if (i == 0) TAKE(idx + 1, 0, v0 < 0.f)
	else if (i == d.sx - 1) TAKE(idx - 1, 0, v0 > 0.f)
	if (j == 0) TAKE(idx + d.Y, 1, v1 < 0.f)
	else if (j == d.sy - 1) TAKE(idx - d.Y, 1, v1 > 0.f)
	if (d.is3d) {
		if (k == 0) TAKE(idx + d.Z, 2, v2 < 0.f)
		else if (k == d.sz - 1) TAKE(idx - d.Z, 2, v2 > 0.f)
	}
#undef TAKE
	if (cnt > 0) {
		const float fc = (float)cnt;
		vel[idx] = v0 / fc;
		vel[n + idx] = v1 / fc;
		vel[2 * n + idx] = v2 / fc;
	}
}
// the loop over the components, fastmarch.cpp:343-366: mark, then `distance` passes
static inline int extrap_component_passes(const Dim& d, const int32_t* flags, float* vel, int distance, int intoObs, int32_t* tmp, hipStream_t st) {
	const int dim = d.is3d ? 3 : 2;
	for (int c = 0; c < dim; c++) {
		hipLaunchKernelGGL(k_extrap_mark, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, flags, tmp, c, intoObs);
		const bool quads = d.is3d && ((((uintptr_t)tmp) & 15) == 0);
		for (int dd = 1; dd < 1 + distance; dd++) {
			if (quads)
				hipLaunchKernelGGL(k_extrap_simple4, dim3((unsigned)((d.n / 4 + BLOCK) / BLOCK)), dim3(BLOCK), 0, st, d, vel + c * d.n, tmp, dd);
			else
				hipLaunchKernelGGL(k_extrap_simple, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, vel + c * d.n, tmp, dd);
		}
	}
	MF_LAUNCH_CHECK();
	return 0;
}
// `MACGrid velTmp; velTmp.copyFrom(vel); knExtrapolateIntoBnd(flags, vel, velTmp)`, fastmarch.cpp:372-374
static inline int extrap_into_bnd(const Dim& d, const int32_t* flags, float* vel, float* velTmp, hipStream_t st) {
	MF_HIP(hipMemcpyAsync(velTmp, vel, sizeof(float) * 3 * d.n, hipMemcpyDeviceToDevice, st));
	hipLaunchKernelGGL(k_extrap_into_bnd, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, flags, vel, velTmp);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // namespace mf
