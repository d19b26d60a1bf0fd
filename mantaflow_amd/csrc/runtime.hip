// runtime.hip -- error reporting, workspace, element-wise grid ops and reductions (gfx950).
#include "reduce.h"
#include <stdarg.h>
#include <float.h>

namespace mf {
thread_local char g_err[512];
thread_local int g_slab_zoff = 0, g_slab_gsz = 0;
thread_local int g_slab_src_zoff = 0, g_slab_src_gsz = 0;
int fail(const char* fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	return 1;
}

// The current device's index into the per-device tables.  What those tables assume: host state per device is shared by the host
// threads of a process, and calls on one device are expected from one thread at a time (the tables are not locked).  Only the error
// text, the slab window, the event pairs of the PCG loop and g_last_shortcut are per thread.
int device_slot(int* slot) {
	int dev = 0;
	MF_HIP(hipGetDevice(&dev));
	if (dev < 0 || dev >= MAX_DEVICES) return fail("device index %d out of range", dev);
	*slot = dev;
	return 0;
}

static Workspace g_ws[MAX_DEVICES];
static bool g_ws_ok[MAX_DEVICES];
// the five allocations of a device's workspace, committed to the table only when all of them stand
static int make_workspace(Workspace* w) {
	MF_HIP(hipMalloc((void**)&w->partials, sizeof(double) * MAX_BLOCKS * 4));
	MF_HIP(hipMalloc((void**)&w->fpartials, sizeof(float) * MAX_BLOCKS * 4));
	MF_HIP(hipMalloc(&w->scalars, 4096));
	MF_HIP(hipMemset(w->scalars, 0, 4096));
	MF_HIP(hipHostMalloc(&w->host, 4096, hipHostMallocDefault));
	MF_HIP(hipMalloc((void**)&w->tilework, 4096));
	MF_HIP(hipMemset(w->tilework, 0, 4096));
	MF_HIP(hipDeviceSynchronize());      // once per device: the two fills are done before any stream's kernel accumulates into them
	return 0;
}
int get_workspace(Workspace** out) {
	int slot;
	MF_TRY(device_slot(&slot));
	if (!g_ws_ok[slot]) {
		Workspace w = {};
		if (make_workspace(&w)) {      // (what was never allocated is null, which hipFree / hipHostFree accept)
			for (void* q : {(void*)w.partials, (void*)w.fpartials, w.scalars, (void*)w.tilework}) (void)hipFree(q);
			(void)hipHostFree(w.host);
			return 1;
		}
		g_ws[slot] = w;
		g_ws_ok[slot] = true;
	}
	*out = &g_ws[slot];
	return 0;
}

int arena_reserve(Arena* per_device, size_t need, Arena** out, bool* regrown) {
	if (regrown) *regrown = false;
	int slot;
	MF_TRY(device_slot(&slot));
	Arena& a = per_device[slot];
	*out = &a;
	if (need > a.cap) {
		const size_t cap = a.cap * 2 > need ? a.cap * 2 : need;
		MF_HIP(hipDeviceSynchronize());
		if (regrown) *regrown = true;
		if (a.p) MF_HIP(hipFree(a.p));
		a.p = nullptr;
		a.cap = 0;
		char* p = nullptr;
		MF_HIP(hipMalloc((void**)&p, cap));
		a.p = p;
		a.cap = cap;
	}
	return 0;
}
}  // namespace mf

using namespace mf;

// ---------------------------------------------------------------------------------------------------------
// element-wise kernels: grid-stride, float4 where the pointers allow it (all grids are 16-B aligned torch
// allocations; the scalar tail handles n % 4 and misaligned views)
// ---------------------------------------------------------------------------------------------------------
enum Op1 { OP_FILL, OP_ADDC, OP_MULC, OP_CLAMP, OP_STOMP };
template <int OP>
__device__ __forceinline__ float op1(float a, float p, float q) {
	if (OP == OP_FILL) return p;
	if (OP == OP_ADDC) return a + p;
	if (OP == OP_MULC) return a * p;
	if (OP == OP_CLAMP) return a < p ? p : (a > q ? q : a);  // general.h:137-141
	if (OP == OP_STOMP) return a < p ? 0.f : a;               // grid.cpp:247
	return a;
}
template <int OP>
__global__ void __launch_bounds__(BLOCK) k_unary(int64_t n, float* __restrict__ a, float p, float q) {
	const int64_t n4 = n >> 2;
	float4* a4 = (float4*)a;
	for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
		float4 v = (OP == OP_FILL) ? make_float4(0, 0, 0, 0) : a4[i];
		v.x = op1<OP>(v.x, p, q);
		v.y = op1<OP>(v.y, p, q);
		v.z = op1<OP>(v.z, p, q);
		v.w = op1<OP>(v.w, p, q);
		a4[i] = v;
	}
	if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
		const int64_t i = (n4 << 2) + threadIdx.x;
		a[i] = op1<OP>(OP == OP_FILL ? 0.f : a[i], p, q);
	}
}
enum Op2 { OP_COPY, OP_AXPY, OP_XPAY, OP_ADD, OP_SUB, OP_MUL, OP_SAFEDIV };
template <int OP>
__device__ __forceinline__ float op2(float a, float b, float f) {
	if (OP == OP_COPY) return b;
	if (OP == OP_AXPY) return a + f * b;               // gridScaledAdd, grid.h:514
	if (OP == OP_XPAY) return b + f * a;               // UpdateSearchVec, conjugategrad.cpp:195
	if (OP == OP_ADD) return a + b;
	if (OP == OP_SUB) return a - b;
	if (OP == OP_MUL) return a * b;
	if (OP == OP_SAFEDIV) return (b != 0.f) ? (a / b) : a;  // general.h:150
	return a;
}
template <int OP>
__global__ void __launch_bounds__(BLOCK) k_binary(int64_t n, float* __restrict__ a, const float* __restrict__ b, float f) {
	const int64_t n4 = n >> 2;
	float4* a4 = (float4*)a;
	const float4* b4 = (const float4*)b;
	for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
		float4 v = (OP == OP_COPY) ? make_float4(0, 0, 0, 0) : a4[i];
		const float4 w = b4[i];
		v.x = op2<OP>(v.x, w.x, f);
		v.y = op2<OP>(v.y, w.y, f);
		v.z = op2<OP>(v.z, w.z, f);
		v.w = op2<OP>(v.w, w.w, f);
		a4[i] = v;
	}
	if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
		const int64_t i = (n4 << 2) + threadIdx.x;
		a[i] = op2<OP>(OP == OP_COPY ? 0.f : a[i], b[i], f);
	}
}
template <int OP>
__global__ void __launch_bounds__(BLOCK) k_unary_scalar(int64_t n, float* a, float p, float q) {
	for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
		a[i] = op1<OP>(OP == OP_FILL ? 0.f : a[i], p, q);
}
template <int OP>
__global__ void __launch_bounds__(BLOCK) k_binary_scalar(int64_t n, float* a, const float* b, float f) {
	for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
		a[i] = op2<OP>(OP == OP_COPY ? 0.f : a[i], b[i], f);
}

template <int OP>
static int run_unary(int64_t n, float* a, float p, float q, void* stream) {
	if (n <= 0) return 0;
	if (al16(a))
		hipLaunchKernelGGL(k_unary<OP>, dim3(blocks_for(n >> 2, BLOCK, 2048)), dim3(BLOCK), 0, (hipStream_t)stream, n, a, p, q);
	else
		hipLaunchKernelGGL(k_unary_scalar<OP>, dim3(blocks_for(n, BLOCK, 2048)), dim3(BLOCK), 0, (hipStream_t)stream, n, a, p, q);
	MF_LAUNCH_CHECK();
	return 0;
}
template <int OP>
static int run_binary(int64_t n, float* a, const float* b, float f, void* stream) {
	if (n <= 0) return 0;
	if (al16(a) && al16(b))
		hipLaunchKernelGGL(k_binary<OP>, dim3(blocks_for(n >> 2, BLOCK, 2048)), dim3(BLOCK), 0, (hipStream_t)stream, n, a, b, f);
	else
		hipLaunchKernelGGL(k_binary_scalar<OP>, dim3(blocks_for(n, BLOCK, 2048)), dim3(BLOCK), 0, (hipStream_t)stream, n, a, b, f);
	MF_LAUNCH_CHECK();
	return 0;
}

// ---------------------------------------------------------------------------------------------------------
// reductions: per-block partials in fixed order -> one finishing block; deterministic run to run
// ---------------------------------------------------------------------------------------------------------
// the terms; DotTerm (GridDotProduct) is in reduce.h
// sum of squares of the value converted to fp64 (GridSumSqr, commonkernels.h:32-35)
struct SumSqrTerm {
	const float* a;
	__device__ __forceinline__ void operator()(int64_t i, double (&acc)[1]) const {
		const double v = (double)a[i];
		acc[0] += v * v;
	}
};
// CompMinReal / CompMaxReal, grid.cpp:185-196
struct MinMaxTerm {
	const float* a;
	__device__ __forceinline__ void operator()(int64_t i, Pair<float> (&acc)[1]) const { MinMaxF32::fold(acc[0], a[i]); }
};
// CompMaxVec, grid.cpp:218-224 : max of normSquare (x*x + y*y + z*z, vectorbase.h:392-395)
struct NormSqTerm {
	const float* a;
	int64_t n;
	__device__ __forceinline__ void operator()(int64_t i, Pair<float> (&acc)[1]) const {
		const float x = a[i], y = a[n + i], z = a[2 * n + i];
		MinMaxF32::fold(acc[0], x * x + y * y + z * z);
	}
};
struct CountFlagTerm {
	const int32_t* f;
	int mask;
	__device__ __forceinline__ void operator()(int64_t i, double (&acc)[1]) const {
		if (f[i] & mask) acc[0] += 1.0;
	}
};

// device-scalar variants (multi-GPU PCG: no host round trip between a reduction and the vector update that uses it)
template <int OP>
__global__ void __launch_bounds__(BLOCK) k_binary_devf(int64_t n, float* a, const float* b, const float* __restrict__ fdev, float sign) {
	const float f = sign * fdev[0];   // sign is +-1: exact
	for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
		a[i] = op2<OP>(a[i], b[i], f);
}

// z-slab PCG scalar steps (common.h: slab_alpha, slab_beta_stop) on loose device scalars
__global__ void k_slab_alpha(const double* __restrict__ g, int world, const float* __restrict__ sigma, float* __restrict__ alpha,
                             const int32_t* __restrict__ state) {
	if (state && state[0]) {
		alpha[0] = 0.f;
		alpha[1] = -0.f;
		return;
	}
	const float a = slab_alpha(g, world, sigma[0]);
	alpha[0] = a;
	alpha[1] = -a;      // nalpha of the CgScalars layout (mf_cg_slab_axpy2)
}
__global__ void k_slab_beta(const double* __restrict__ g, int world, float* __restrict__ sigma, float* __restrict__ beta, float* __restrict__ res,
                            float accuracy, int iter, int32_t* __restrict__ state) {
	if (state && state[0]) return;
	const SlabBeta b = slab_beta_stop(g, world, sigma[0], accuracy);
	res[0] = b.resNorm;
	beta[0] = b.beta;
	sigma[0] = b.sigmaNew;
	if (state && b.stop) {
		state[0] = b.stop;
		state[1] = iter;
	}
}
int mf::launch_sum_finish(int nb, const double* partials, double* out, hipStream_t st) {
	return reduce_finish<SumF64, 1>(nb, 1, partials, Store<double>{out}, st);
}
int mf::launch_maxabs_finish(int nb, const float* fpart, double* out, const int* stopped, hipStream_t st) {
	return reduce_finish<MinMaxF32, 1>(nb, 1, (const Pair<float>*)fpart, StoreMaxAbs<double>{out, stopped}, st);
}

int mf::read_back(void* host, const void* dev, size_t bytes, hipStream_t st) {
	MF_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
	MF_HIP(hipStreamSynchronize(st));
	return 0;
}
int mf::read_scalars(Workspace* ws, const void* dev, size_t bytes, void* host_out, hipStream_t s) {
	MF_TRY(read_back(ws->host, dev, bytes, s));
	memcpy(host_out, ws->host, bytes);
	return 0;
}

// this file's reductions: blocks_for(n, BLOCK * 8, 1024) blocks, partials in the workspace.  The sum goes to out_dev, or (null) through
// the workspace's scalar block to out_host
template <class Term>
static int sum_of(int64_t n, Term term, double* out_dev, double* out_host, void* s) {
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	double* out = out_dev ? out_dev : (double*)ws->scalars;
	MF_TRY((reduce<SumF64, 1>(n, dim3(blocks_for(n, BLOCK * 8, 1024)), term, ws->partials, Store<double>{out}, (hipStream_t)s)));
	return out_dev ? 0 : read_scalars(ws, out, sizeof(double), out_host, (hipStream_t)s);
}
// max |.| of the minimum and the maximum to maxabs_dev, or (null) the two themselves to lohi_host
template <class Term, class O>
static int minmax_of(int64_t n, Term term, O* maxabs_dev, float* lohi_host, void* s) {
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const dim3 grid(blocks_for(n, BLOCK * 8, 1024));
	Pair<float>*part = (Pair<float>*)ws->fpartials, *out = (Pair<float>*)ws->scalars;
	if (maxabs_dev) return reduce<MinMaxF32, 1>(n, grid, term, part, StoreMaxAbs<O>{maxabs_dev, nullptr}, (hipStream_t)s);
	MF_TRY((reduce<MinMaxF32, 1>(n, grid, term, part, Store<Pair<float>>{out}, (hipStream_t)s)));
	return read_scalars(ws, out, sizeof(*out), lohi_host, (hipStream_t)s);
}

extern "C" {

const char* mf_last_error(void) { return mf::g_err; }
const char* mf_backend(void) { return "hip"; }
int mf_abi_version(void) { return MF_ABI_VERSION; }
int mf_set_slab_window(int zoff, int gsz) {
	if (gsz < 0 || zoff < 0 || (gsz > 0 && zoff >= gsz)) return fail("invalid slab window %d / %d", zoff, gsz);
	mf::g_slab_zoff = zoff;
	mf::g_slab_gsz = gsz;
	return 0;
}
int mf_set_slab_window_source(int zoff, int gsz) {
	if (gsz < 0 || zoff < 0 || (gsz > 0 && zoff >= gsz)) return fail("invalid source slab window %d / %d", zoff, gsz);
	mf::g_slab_src_zoff = zoff;
	mf::g_slab_src_gsz = gsz;
	return 0;
}

int mf_fill_f32(int64_t n, float* a, float v, void* s) { return run_unary<OP_FILL>(n, a, v, 0.f, s); }
int mf_fill_i32(int64_t n, int32_t* a, int32_t v, void* s) {
	float f;
	memcpy(&f, &v, 4);
	return run_unary<OP_FILL>(n, (float*)a, f, 0.f, s);
}
int mf_copy_f32(int64_t n, float* dst, const float* src, void* s) {
	if (n <= 0) return 0;
	MF_HIP(hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyDeviceToDevice, (hipStream_t)s));
	return 0;
}
int mf_grid_scaled_add(int64_t n, float* me, const float* o, float f, void* s) { return run_binary<OP_AXPY>(n, me, o, f, s); }
int mf_update_search_vec(int64_t n, float* dst, const float* src, float f, void* s) { return run_binary<OP_XPAY>(n, dst, src, f, s); }
int mf_grid_add(int64_t n, float* me, const float* o, void* s) { return run_binary<OP_ADD>(n, me, o, 0.f, s); }
int mf_grid_sub(int64_t n, float* me, const float* o, void* s) { return run_binary<OP_SUB>(n, me, o, 0.f, s); }
int mf_grid_mult(int64_t n, float* me, const float* o, void* s) { return run_binary<OP_MUL>(n, me, o, 0.f, s); }
int mf_grid_safe_divide(int64_t n, float* me, const float* o, void* s) { return run_binary<OP_SAFEDIV>(n, me, o, 0.f, s); }
int mf_grid_stomp(int64_t n, float* a, float th, void* s) { return run_unary<OP_STOMP>(n, a, th, 0.f, s); }
int mf_grid_add_const(int64_t n, float* a, float v, void* s) { return run_unary<OP_ADDC>(n, a, v, 0.f, s); }
int mf_grid_mult_const(int64_t n, float* a, float v, void* s) { return run_unary<OP_MULC>(n, a, v, 0.f, s); }
int mf_grid_clamp(int64_t n, float* a, float lo, float hi, void* s) { return run_unary<OP_CLAMP>(n, a, lo, hi, s); }

int mf_grid_dot(int64_t n, const float* a, const float* b, double* r, void* s) { return sum_of(n, DotTerm{a, b}, nullptr, r, s); }
int mf_grid_dot_dev(int64_t n, const float* a, const float* b, double* out_dev, void* s) { return sum_of(n, DotTerm{a, b}, out_dev, nullptr, s); }
int mf_grid_max_abs_dev(int64_t n, const float* a, float* out_dev, void* s) { return minmax_of(n, MinMaxTerm{a}, out_dev, nullptr, s); }
int mf_grid_max_abs_dev_f64(int64_t n, const float* a, double* out_dev, void* s) { return minmax_of(n, MinMaxTerm{a}, out_dev, nullptr, s); }
int mf_cg_slab_alpha(const double* gathered, int world, const float* sigma_dev, float* alpha_dev, const int32_t* state_dev, void* s) {
	hipLaunchKernelGGL(k_slab_alpha, dim3(1), dim3(1), 0, (hipStream_t)s, gathered, world, sigma_dev, alpha_dev, state_dev);
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_cg_slab_beta(const double* gathered, int world, float* sigma_dev, float* beta_dev, float* res_dev, float accuracy, int iter,
                    int32_t* state_dev, void* s) {
	hipLaunchKernelGGL(k_slab_beta, dim3(1), dim3(1), 0, (hipStream_t)s, gathered, world, sigma_dev, beta_dev, res_dev, accuracy, iter, state_dev);
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_grid_scaled_add_dev(int64_t n, float* me, const float* o, const float* factor_dev, float sign, void* s) {
	if (n <= 0) return 0;
	hipLaunchKernelGGL(k_binary_devf<OP_AXPY>, dim3(blocks_for(n, BLOCK * 4, 4096)), dim3(BLOCK), 0, (hipStream_t)s, n, me, o, factor_dev, sign);
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_update_search_vec_dev(int64_t n, float* dst, const float* src, const float* factor_dev, void* s) {
	if (n <= 0) return 0;
	hipLaunchKernelGGL(k_binary_devf<OP_XPAY>, dim3(blocks_for(n, BLOCK * 4, 4096)), dim3(BLOCK), 0, (hipStream_t)s, n, dst, src, factor_dev, 1.f);
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_grid_sum_sqr(int64_t n, const float* a, double* r, void* s) { return sum_of(n, SumSqrTerm{a}, nullptr, r, s); }
int mf_grid_min_max(int64_t n, const float* a, float* mn, float* mx, void* s) {
	float r[2];
	MF_TRY(minmax_of(n, MinMaxTerm{a}, (float*)nullptr, r, s));
	*mn = r[0];
	*mx = r[1];
	return 0;
}
int mf_grid_max_abs(int64_t n, const float* a, float* r, void* s) {
	float lo, hi;
	MF_TRY(mf_grid_min_max(n, a, &lo, &hi, s));
	*r = maxabs(lo, hi);
	return 0;
}
int mf_grid_max_abs_vec3(int64_t n, const float* a, float* r, void* s) {
	float v[2];
	MF_TRY(minmax_of(n, NormSqTerm{a, n}, (float*)nullptr, v, s));
	*r = sqrtf(v[1]);
	return 0;
}
int mf_count_empty_cells(int64_t n, const int32_t* flags, int32_t* r, void* s) {
	double d;
	MF_TRY(sum_of(n, CountFlagTerm{flags, (int)MF_EMPTY}, nullptr, &d, s));
	*r = (int32_t)d;
	return 0;
}

}  // extern "C"
