// fields.hip -- the fire, wave-equation and uv-grid plugins (include/open/manta_hip_fields.h): pure grid code, one thread per cell
// with lanes along x; the per-cell bodies are in fields_cells.h.
// Reference: plugin/fire.cpp, plugin/waves.cpp, grid.cpp:573-627, plugin/waveletturbulence.cpp:239-307, plugin/initplugins.cpp:478-503.
#include "fields_cells.h"
#include "reduce.h"
#include "../../include/open/manta_hip_fields.h"

using namespace mf;
using namespace mf::fields;

namespace {

__global__ void __launch_bounds__(BLOCK)
k_process_burn(Dim d, float* fuel, float* density, float* react, float* red, float* green, float* blue, float* heat, Burn B) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	process_burn(idx, fuel, density, react, red, green, blue, heat, B);
}

__global__ void __launch_bounds__(BLOCK) k_update_flame(Dim d, const float* __restrict__ react, float* __restrict__ flame) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	flame[idx] = update_flame(react[idx]);
}

__global__ void __launch_bounds__(BLOCK) k_sec_deriv_2d(Dim d, const float* __restrict__ v, float* __restrict__ ret) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	ret[idx] = (float)five_point(d, v, idx);
}

// knTotalSum, waves.cpp:46-47: the fp64 sum of the interior cells in the fixed order of reduce.h; the epilogue leaves the sum as a
// double and, one double further, rounded to Real
struct InteriorTerm {
	Dim d;
	const float* h;
	__device__ __forceinline__ void operator()(int64_t idx, double (&acc)[1]) const {
		int i, j, k;
		cell_ijk(d, idx, i, j, k);
		if (INTERIOR(d)) acc[0] += (double)h[idx];
	}
};
struct StoreSum32 {
	double* sum;
	__device__ __forceinline__ void operator()(const double (&acc)[1]) const {
		sum[0] = acc[0];
		*(float*)(sum + 1) = (float)acc[0];
	}
};
// `Real factor = target / ts.sum; height.multConst(factor)`, waves.cpp:58-59: a double quotient rounded once, from the device scalar
__global__ void __launch_bounds__(BLOCK) k_scale_to(int64_t n, float* __restrict__ h, float target, const double* __restrict__ sum) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	const float factor = (float)((double)target / *sum);
	h[idx] *= factor;
}

__global__ void __launch_bounds__(BLOCK)
k_wave_system(Dim d, float* A0, float* Ai, float* Aj, float* Ak, float* rhs, const float* __restrict__ ut, const float* __restrict__ utm1, float s,
              int crankNic) {
	CELL_IJK(d)
	wave_system(d, idx, INTERIOR(d), A0, Ai, Aj, Ak, rhs, ut, utm1, s, crankNic);
}

__global__ void __launch_bounds__(BLOCK) k_reset_uv(Dim d, float* __restrict__ uv, float ox, float oy, float oz) {
	CELL_IJK(d)
	uv[idx] = (float)i + ox;
	uv[d.n + idx] = (float)j + oy;
	uv[2 * d.n + idx] = (float)k + oz;
}
__global__ void k_set_uv_weight(int64_t n, float* __restrict__ uv, float w) {
	if (blockIdx.x == 0 && threadIdx.x < 3) uv[threadIdx.x * n] = threadIdx.x == 0 ? w : 0.f;
}

__global__ void __launch_bounds__(BLOCK) k_extrapolate_mark(int64_t n, const int32_t* __restrict__ flags, int32_t* __restrict__ tmp, int flagFrom) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	tmp[idx] = (flags[idx] & flagFrom) ? 1 : 0;
}
// tmp and val are read at the neighbours and written at the cell itself by the same launch: see the header for why that is order-free
template <class T>
__global__ void __launch_bounds__(BLOCK) k_extrapolate_pass(Dim d, const int32_t* __restrict__ flags, int32_t* tmp, T* val, int ncomp, int dist, int flagTo) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	extrapolate_cell<T>(d, idx, flags, tmp, val, ncomp, dist, flagTo);
}

int interior_sum(const Dim& d, const float* h, Workspace* ws, hipStream_t st) {
	return reduce<SumF64, 1>(d.n, dim3(blocks_for(d.n, BLOCK * 8, 1024)), InteriorTerm{d, h}, ws->partials, StoreSum32{(double*)ws->scalars}, st);
}

}  // namespace

extern "C" {

int mf_fields_abi_version(void) { return MF_FIELDS_ABI_VERSION; }

int mf_fields_process_burn(int sx, int sy, int sz, float* fuel, float* density, float* react, float* red, float* green, float* blue,
                           float* heat, float burningRate, float flameSmoke, float ignitionTemp, float maxTemp, float dt, float colorX,
                           float colorY, float colorZ, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	const Burn B = {burningRate, flameSmoke, ignitionTemp, maxTemp, dt, colorX, colorY, colorZ};
	hipLaunchKernelGGL(k_process_burn, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, fuel, density, react, red, green, blue, heat, B);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_fields_update_flame(int sx, int sy, int sz, const float* react, float* flame, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_update_flame, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, react, flame);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_fields_sec_deriv_2d(int sx, int sy, int sz, const float* v, float* ret, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (v == ret) return fail("calcSecDeriv2d: curv must not alias v");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_sec_deriv_2d, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, v, ret);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_fields_total_sum(int sx, int sy, int sz, const float* h, float* sum_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const hipStream_t st = (hipStream_t)stream;
	MF_TRY(interior_sum(mkdim(sx, sy, sz), h, ws, st));
	return read_scalars(ws, (double*)ws->scalars + 1, sizeof(float), sum_host, st);
}

int mf_fields_normalize_sum(int sx, int sy, int sz, float* h, float target, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const hipStream_t st = (hipStream_t)stream;
	const Dim d = mkdim(sx, sy, sz);
	MF_TRY(interior_sum(d, h, ws, st));
	hipLaunchKernelGGL(k_scale_to, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d.n, h, target, (const double*)ws->scalars);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_fields_wave_system(int sx, int sy, int sz, float* A0, float* Ai, float* Aj, float* Ak, float* rhs, const float* ut,
                          const float* utm1, float s, int crankNic, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_wave_system, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, A0, Ai, Aj, Ak, rhs, ut, utm1, s, crankNic);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_fields_reset_uv(int sx, int sy, int sz, float* uv, float offX, float offY, float offZ, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_reset_uv, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, uv, offX, offY, offZ);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_fields_set_uv_weight(int64_t n, float* uv, float w, void* stream) {
	if (n < 1) return fail("mf_fields_set_uv_weight: invalid size");
	hipLaunchKernelGGL(k_set_uv_weight, dim3(1), dim3(64), 0, (hipStream_t)stream, n, uv, w);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_fields_get_uv_weight(const float* uv, float* w_host, void* stream) {
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	return read_scalars(ws, uv, sizeof(float), w_host, (hipStream_t)stream);
}

int mf_fields_extrapolate_mark(int64_t n, const int32_t* flags, int32_t* tmp, int flagFrom, void* stream) {
	if (n < 0) return fail("mf_fields_extrapolate_mark: negative size");
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_extrapolate_mark, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, flags, tmp, flagFrom);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_fields_extrapolate_pass(int sx, int sy, int sz, const int32_t* flags, int32_t* tmp, void* val, int ncomp, int isInt, int d,
                               int flagTo, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if ((ncomp != 1 && ncomp != 3) || (isInt && ncomp != 1) || d < 1) return fail("mf_fields_extrapolate_pass: invalid ncomp %d / isInt %d / d %d", ncomp, isInt, d);
	const Dim dm = mkdim(sx, sy, sz);
	if (isInt)
		hipLaunchKernelGGL(k_extrapolate_pass<int32_t>, dim3(nblk(dm.n)), dim3(BLOCK), 0, (hipStream_t)stream, dm, flags, tmp, (int32_t*)val, 1, d, flagTo);
	else
		hipLaunchKernelGGL(k_extrapolate_pass<float>, dim3(nblk(dm.n)), dim3(BLOCK), 0, (hipStream_t)stream, dm, flags, tmp, (float*)val, ncomp, d, flagTo);
	MF_LAUNCH_CHECK();
	return 0;
}

// kninitVortexVelocity, initplugins.cpp:479-499, on the host: `i - center.x` is int - Real, `-= .5` a double subtraction rounded into
// the Real (exact), std::sqrt / atan2 / std::sin / std::cos resolve to the float overloads
int mf_fields_vortex_velocity(int sx, int sy, int sz, const float* phiObs, float* vel, float centerX, float centerY, float radius) {
	MF_TRY(check_dim(sx, sy, sz));
	const int64_t n = (int64_t)sx * sy * sz;
	for (int k = 0; k < sz; k++)
		for (int j = 0; j < sy; j++)
			for (int i = 0; i < sx; i++) {
				const int64_t idx = i + (int64_t)sx * (j + (int64_t)sy * k);
				if (!((double)phiObs[idx] >= -1.)) continue;
				float dx = (float)i - centerX;
				if (dx >= 0) dx = (float)((double)dx - .5);
				else dx = (float)((double)dx + .5);
				float dy = (float)j - centerY;
				float r = sqrtf(dx * dx + dy * dy);
				float alpha = atan2f(dy, dx);
				vel[idx] = -sinf(alpha) * (r / radius);
				dx = (float)i - centerX;
				dy = (float)j - centerY;
				if (dy >= 0) dy = (float)((double)dy - .5);
				else dy = (float)((double)dy + .5);
				r = sqrtf(dx * dx + dy * dy);
				alpha = atan2f(dy, dx);
				vel[n + idx] = cosf(alpha) * (r / radius);
			}
	return 0;
}

}  // extern "C"
