// guiding.hip -- primal-dual fluid guiding, source/plugin/fluidguiding.cpp (include/manta_hip_guiding.h): the Gaussian weights
// (:31-45, host), the separable blur with its obstacle restore (:49-136), precomputeInvA (:254-263) and the element-wise chains of
// one primal-dual iteration (:229-239, :266-271, :323-344) in three kernels.  DESIGN.md, "Primal-dual fluid guiding", has the
// rounding points and the forms of the blur that were considered.
#include "reduce.h"
#include "../../include/manta_hip_guiding.h"
#include <math.h>

using namespace mf;

namespace {

// ---- blur -------------------------------------------------------------------------------------------------------------------------
// apply1DKernelDirX/Y/Z (:49-84), one thread per cell, the three components at the cell's own index; taps come from the caches
// (neighbouring lanes read neighbouring taps along x, the same rows shifted along y and z).  The reference walks m = 0 .. kn-1 with
// ii = pos - kn/2 + m, skipping ii < 0 and leaving at ii >= len: that is m = lo .. hi below, in the same order, on an accumulator that
// starts at 0.  LAST: the pass writes the blurred grid itself, which still holds the values from before the blur, so the restore of
// :99-105 / :123-129 is "leave the cell alone".
template <int AXIS, bool LAST>
__global__ void __launch_bounds__(BLOCK)
k_guiding_blur(Dim d, const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ w, int radius,
               const int32_t* __restrict__ flags) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= d.n) return;
	const int i = (int)(idx % d.sx);
	const int j = (int)((idx / d.sx) % d.sy);
	const int k = (int)(idx / ((int64_t)d.sx * d.sy));
	if (LAST) {
		const bool keep = (flags[idx] & MF_OBSTACLE) || (i > 0 && (flags[idx - 1] & MF_OBSTACLE)) || (j > 0 && (flags[idx - d.Y] & MF_OBSTACLE)) ||
		                  (d.is3d && k > 0 && (flags[idx - d.Z] & MF_OBSTACLE));
		if (keep) return;
	}
	const int pos = AXIS == 0 ? i : (AXIS == 1 ? j : k);
	const int len = AXIS == 0 ? d.sx : (AXIS == 1 ? d.sy : d.sz);
	const int64_t stride = AXIS == 0 ? 1 : (AXIS == 1 ? (int64_t)d.sx : (int64_t)d.sx * d.sy);
	const int kn = 2 * radius + 1;
	const int lo = radius - pos > 0 ? radius - pos : 0;
	const int hi = len - 1 - pos + radius < kn - 1 ? len - 1 - pos + radius : kn - 1;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const float* p = in + c * d.n + idx + (int64_t)(lo - radius) * stride;
		float acc = 0.f;
		for (int m = lo; m <= hi; m++, p += stride) {
			const float t = *p * w[kn - 1 - m];
			acc += t;
		}
		out[c * d.n + idx] = acc;
	}
}

template <int AXIS, bool LAST>
int blur_pass(const Dim& d, const float* in, float* out, const float* w, int radius, const int32_t* flags, hipStream_t st) {
	hipLaunchKernelGGL((k_guiding_blur<AXIS, LAST>), dim3((unsigned)((d.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, d, in, out, w, radius, flags);
	MF_LAUNCH_CHECK();
	return 0;
}

// ---- element-wise -----------------------------------------------------------------------------------------------------------------
// one thread per cell and its three components; every line is one rounding of the reference's chain of grid methods
__global__ void __launch_bounds__(BLOCK) k_guiding_inv_a(int64_t n, const float* __restrict__ weight, float sigma, float* __restrict__ invA) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	const float wv = weight[idx];
	float val = 2.f * wv * wv + sigma;                  // Real val = 2 * w * w + sigma
	if ((double)val < 0.01) val = (float)0.01;          // compared against the double literal
	invA[idx] = (float)(1.0 / (double)val);
}

__global__ void __launch_bounds__(BLOCK)
k_guiding_pre(int64_t n, const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ Q, const float* __restrict__ invA,
              float* __restrict__ xv, float* __restrict__ vn, float inv_sigma, float sigma) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	const float a = invA[idx];
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const int64_t q = c * n + idx;
		float v = x[q] * inv_sigma;   // x.multConst(1.0 / sigma)
		v = v + y[q];                 // x.add(y)
		v = v * sigma;                // prox_f: v.multConst(sigma)
		v = v + Q[q];                 //         v.add(Q)
		xv[q] = v;
		vn[q] = v * a;                // applyApproxInvM: v_new = v * invA
	}
}

__global__ void __launch_bounds__(BLOCK)
k_guiding_mid(int64_t n, float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ xv, const float* __restrict__ vn,
              const float* __restrict__ invA, const float* __restrict__ velC, const float* __restrict__ z, float* __restrict__ zn, float sigma,
              float tau) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	const float a = invA[idx];
	const float nsigma = -sigma, ntau = -tau;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const int64_t q = c * n + idx;
		float b = vn[q] * 2.f;        // v_new.multConst(2.0)
		b = b * a;                    // v_new.mult(invA)
		float v = xv[q] * a;          // v.mult(invA)
		v = v - b;                    // v.sub(v_new)
		v = v + velC[q];              // prox_f: v.add(velC)
		v = v * nsigma;               // x.multConst(-sigma)
		const float sy = sigma * y[q];
		v = v + sy;                   // x.addScaled(y, sigma)
		v = v + x[q];                 // x.add(x0)
		x[q] = v;
		const float tx = ntau * v;
		zn[q] = z[q] + tx;            // z.addScaled(x, -tau)
	}
}

// y = ((z - z0) * theta) + z, and per block the largest normSquare of z - z0 and of z (vectorbase.h:392-395: x*x + y*y + z*z)
__global__ void __launch_bounds__(BLOCK)
k_guiding_post(int64_t n, const float* __restrict__ z, const float* __restrict__ z0, float* __restrict__ y, float theta, Pair<float>* __restrict__ partials) {
	float mr = -FLT_MAX, mz = -FLT_MAX;
	for (int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * BLOCK) {
		float r[3], zz[3];
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const int64_t q = c * n + idx;
			zz[c] = z[q];
			r[c] = zz[c] - z0[q];
			const float t = r[c] * theta;
			y[q] = t + zz[c];
		}
		mr = fmaxf(mr, r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
		mz = fmaxf(mz, zz[0] * zz[0] + zz[1] * zz[1] + zz[2] * zz[2]);
	}
	// the loop writes y, so the kernel is its own; its two maxima ride the shared min / max fold in one pass, the first one negated as the
	// minimum (negation is exact, and fminf(-a, -b) is -fmaxf(a, b)): a max / max pair policy for this one caller would be more code than
	// the two negations, here and in the finisher's epilogue
	const Pair<float> r = block_fold<MinMaxF32>({-mr, mz});
	if (threadIdx.x == 0) partials[blockIdx.x] = r;
}
struct StoreNegLo {
	float* out;
	__device__ __forceinline__ void operator()(const Pair<float> (&acc)[1]) const {
		out[0] = -acc[0].lo;
		out[1] = acc[0].hi;
	}
};

int check_n(const char* who, int64_t n) {
	if (n < 1 || 3 * n >= (int64_t)1 << 31) return fail("%s: invalid cell count %lld", who, (long long)n);
	if (g_slab_gsz > 0) return fail("%s: not available inside a z-slab window", who);
	return 0;
}

// Matrix::add_to_element / operator() (util/rcmatrix.h:175-206): a value with |v| <= 1e-6f is never stored and reads back as 0
inline float sparse(float v) { return fabsf(v) > 1e-6f ? v : 0.f; }

}  // namespace

extern "C" {

int mf_guiding_abi_version(void) { return MF_GUIDING_ABI_VERSION; }

int mf_guiding_weights(int radius, float* w) {
	if (radius < 0 || radius > 1024) return fail("mf_guiding_weights: invalid radius %d", radius);
	if (!w) return fail("mf_guiding_weights: no output");
	const int n = 2 * radius + 1, sigma = n;
	float sumG = 0.f;            // Real sumG
	for (int j = 0; j < n; j++) {
		const float x = sparse((float)(-(n - 1) * 0.5));      // the same entry for every tap, as the reference has it
		const float y = sparse((float)(j - (n - 1) * 0.5));
		const float xx = x * x, yy = y * y;
		const float s = xx + yy;
		const float arg = -s / (float)(2 * sigma * sigma);    // Real / int
		const float e = expf(arg);                            // exp(float): the float overload
		const double g = 1 / (2 * M_PI * sigma * sigma) * (double)e;
		w[j] = sparse((float)g);
		sumG = sumG + w[j];
	}
	const double kf = 1.0 / (double)sumG;                     // G * (1.0 / sumG): RCMatrix::operator*(double)
	for (int j = 0; j < n; j++)
		if (w[j] != 0.f) w[j] = sparse((float)((double)w[j] * kf));
	return 0;
}

int mf_guiding_blur(int sx, int sy, int sz, const int32_t* flags, float* grid, float* s1, float* s2, const float* w_dev, int radius,
                    int times, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	MF_TRY(check_n("mf_guiding_blur", (int64_t)sx * sy * sz));
	if (radius < 0 || radius > 1024) return fail("mf_guiding_blur: invalid radius %d", radius);
	const Dim d = mkdim(sx, sy, sz);
	if (!flags || !grid || !s1 || !w_dev || (d.is3d && !s2)) return fail("mf_guiding_blur: missing grid, scratch or weights");
	hipStream_t st = (hipStream_t)stream;
	for (int t = 0; t < times; t++) {
		MF_TRY((blur_pass<0, false>(d, grid, s1, w_dev, radius, flags, st)));
		if (d.is3d) {
			MF_TRY((blur_pass<1, false>(d, s1, s2, w_dev, radius, flags, st)));
			MF_TRY((blur_pass<2, true>(d, s2, grid, w_dev, radius, flags, st)));
		} else {
			MF_TRY((blur_pass<1, true>(d, s1, grid, w_dev, radius, flags, st)));
		}
	}
	return 0;
}

int mf_guiding_inv_a(int64_t n, const float* weight, float sigma, float* invA, void* stream) {
	MF_TRY(check_n("mf_guiding_inv_a", n));
	hipLaunchKernelGGL(k_guiding_inv_a, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, weight, sigma, invA);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_guiding_pre(int64_t n, const float* x, const float* y, const float* Q, const float* invA, float* xv, float* vn, float inv_sigma,
                   float sigma, void* stream) {
	MF_TRY(check_n("mf_guiding_pre", n));
	hipLaunchKernelGGL(k_guiding_pre, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, x, y, Q, invA, xv, vn, inv_sigma, sigma);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_guiding_mid(int64_t n, float* x, const float* y, const float* xv, const float* vn, const float* invA, const float* velC,
                   const float* z, float* zn, float sigma, float tau, void* stream) {
	MF_TRY(check_n("mf_guiding_mid", n));
	hipLaunchKernelGGL(k_guiding_mid, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, x, y, xv, vn, invA, velC, z, zn, sigma, tau);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_guiding_post(int64_t n, const float* z, const float* z0, float* y, float theta, float* out_host, void* stream) {
	MF_TRY(check_n("mf_guiding_post", n));
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	hipStream_t st = (hipStream_t)stream;
	const int nb = blocks_for(n, BLOCK * 4, 2048);
	Pair<float>* part = (Pair<float>*)ws->fpartials;
	hipLaunchKernelGGL(k_guiding_post, dim3(nb), dim3(BLOCK), 0, st, n, z, z0, y, theta, part);
	MF_TRY((reduce_finish<MinMaxF32, 1>(nb, 1, part, StoreNegLo{(float*)ws->scalars}, st)));
	float h[2];
	MF_TRY(read_scalars(ws, ws->scalars, sizeof(h), h, st));
	out_host[0] = sqrtf(h[0]);
	out_host[1] = sqrtf(h[1]);
	return 0;
}

}  // extern "C"
