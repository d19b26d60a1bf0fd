// datagen.hip -- the smoke data-generation plugins (include/open/manta_hip_datagen.h): the Gaussian grid blurs of
// source/plugin/initplugins.cpp:510-655, calcCenterOfMass (:337-348), projectImg with writePpm's byte conversion
// (source/util/simpleimage.cpp:20-67, 206-281), LaplaceOp and CurvatureOp (source/commonkernels.h:75-101).  DESIGN.md section 23 has
// the rounding points.  The reference's Real is float; a literal such as 2.0, 0.5 or 1. makes its expression double until the next
// store into a Real, which is what the casts below say.
#include "reduce.h"
#include "../../include/open/manta_hip_datagen.h"
#include <math.h>

using namespace mf;

namespace {

// ---- blur -------------------------------------------------------------------------------------------------------------------------
// The weights are a kernel argument: the tap loop is uniform, so every w[d] is a scalar load from the kernel-argument segment and no
// device copy of the weights exists (nothing to upload, nothing to wait for).
struct Taps {
	int n;
	float w[MF_DATAGEN_MAX_TAPS];
};

// knBlurGrid / KnBlurMACGridGauss (:570-639), one thread per cell, lanes along x, the NC components at the cell's own index.  The
// reference walks d = 0 .. mDim-1 with curpos = pos - (d - mDim/2) e_AXIS clamped into the grid (only AXIS can leave it); the x pass
// takes its taps from the neighbouring lanes' cells (the caches), the y and z passes read whole rows.  Unlike k_guiding_blur
// (guiding.hip) a tap outside the grid is clamped, not skipped, and nothing is restored afterwards.
template <int AXIS, int NC>
__global__ void __launch_bounds__(BLOCK) k_datagen_blur(Dim d, const float* __restrict__ in, float* __restrict__ out, Taps t) {
	CELL_IJK(d);
	const int pos = AXIS == 0 ? i : (AXIS == 1 ? j : k);
	const int last = (AXIS == 0 ? d.sx : (AXIS == 1 ? d.sy : d.sz)) - 1;
	const int64_t stride = AXIS == 0 ? 1 : (AXIS == 1 ? (int64_t)d.sx : (int64_t)d.sx * d.sy);
	const int c = t.n / 2;
	float acc[NC];
#pragma unroll
	for (int q = 0; q < NC; q++) acc[q] = 0.f;
	for (int m = 0; m < t.n; m++) {
		int p = pos - (m - c);
		p = p < 0 ? 0 : (p > last ? last : p);
		const int64_t at = idx + (int64_t)(p - pos) * stride;
		const float w = t.w[m];
#pragma unroll
		for (int q = 0; q < NC; q++) {
			const float pr = w * in[q * d.n + at];
			acc[q] = acc[q] + pr;
		}
	}
#pragma unroll
	for (int q = 0; q < NC; q++) out[q * d.n + idx] = acc[q];
}

template <int AXIS>
int blur_pass(const Dim& d, int ncomp, const float* in, float* out, const Taps& t, hipStream_t st) {
	if (ncomp == 1)
		hipLaunchKernelGGL((k_datagen_blur<AXIS, 1>), dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, in, out, t);
	else
		hipLaunchKernelGGL((k_datagen_blur<AXIS, 3>), dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, in, out, t);
	MF_LAUNCH_CHECK();
	return 0;
}

// GaussianKernelCreator::setGaussianSigma, :535-557
int make_taps(const char* who, float sigma, int cap, Taps* t) {
	if (!(sigma > 0.f) || !isfinite(sigma)) return fail("%s: sigma must be positive", who);
	const double dd = 2.0 * 3.0 * (double)sigma + (double)1.0f;
	if (dd > (double)cap) return fail("%s: sigma %g needs a kernel of more than %d taps", who, (double)sigma, cap);
	int mDim = (int)dd;
	if (mDim < 3) mDim = 3;
	if (mDim % 2 == 0) ++mDim;
	if (mDim > cap) return fail("%s: sigma %g needs a kernel of more than %d taps", who, (double)sigma, cap);
	const float s2 = sigma * sigma;
	const int c = mDim / 2;
	const float m = (float)(1.0 / (sqrt(2.0 * M_PI) * (double)sigma));
	for (int i = 0; i < (mDim + 1) / 2; i++) {
		const float v = (float)((double)m * exp(-(1.0 * i * i) / (2.0 * (double)s2)));
		t->w[c + i] = v;
		t->w[c - i] = v;
	}
	t->n = mDim;
	return 0;
}

// ---- centre of mass ---------------------------------------------------------------------------------------------------------------
// the four sums: each term is the reference's fp32 product, the sums are fp64 in the fixed order of reduce.h
struct ComTerm {
	Dim d;
	const float* density;
	__device__ __forceinline__ void operator()(int64_t idx, double (&s)[4]) const {
		int i, j, k;
		cell_ijk(d, idx, i, j, k);
		const float v = density[idx];
		const float tx = v * ((float)i + 0.5f), ty = v * ((float)j + 0.5f), tz = v * ((float)k + 0.5f);
		s[0] += (double)tx;
		s[1] += (double)ty;
		s[2] += (double)tz;
		s[3] += (double)v;
	}
};
// the `w > 1e-6f` test on the rounded weight, the quotients
struct ComQuotients {
	float* out;
	__device__ __forceinline__ void operator()(const double (&s)[4]) const {
		const bool divide = (float)s[3] > 1e-6f;
		for (int q = 0; q < 3; q++) out[q] = divide ? (float)(s[q] / s[3]) : (float)s[q];
	}
};

// ---- projection -------------------------------------------------------------------------------------------------------------------
// gridPrecompLight (simpleimage.cpp:206-215) for one cell: n = getGradient * -1. (grid.h:556-573; an exact negation), normalize
// (vectorbase.h:421-434), dot((1, 1, 1), n)
__device__ __forceinline__ float light_of(const Dim& d, const float* __restrict__ val, int i, int j, int k) {
	if (i > d.sx - 2) i = d.sx - 2;
	if (j > d.sy - 2) j = d.sy - 2;
	if (i < 1) i = 1;
	if (j < 1) j = 1;
	const int64_t xy = (int64_t)i + d.Y * j + d.Z * k;
	float gx = -(val[xy + 1] - val[xy - 1]), gy = -(val[xy + d.Y] - val[xy - d.Y]), gz = -0.f;
	if (d.is3d) {
		if (k > d.sz - 2) k = d.sz - 2;
		if (k < 1) k = 1;
		const int64_t at = (int64_t)i + d.Y * j + d.Z * k;
		gz = -(val[at + d.Z] - val[at - d.Z]);
	}
	const float l = gx * gx + gy * gy + gz * gz;
	const float eps2 = 1e-6f * 1e-6f;
	if (fabs((double)l - 1.) < (double)eps2) {
	} else if (l > eps2) {
		const float nrm = sqrtf(l);
		const float fac = (float)(1. / (double)nrm);
		gx *= fac;
		gy *= fac;
		gz *= fac;
	} else {
		gx = gy = gz = 0.f;
	}
	return 1.f * gx + 1.f * gy + 1.f * gz;
}

// the grid L of projectImg, filled only in surface mode (the reference fills it always and reads it only there): one thread per cell,
// lanes along x.  Forming the light inside the views instead made the x view 4.7 times as slow as the z view at 256^3 (its six
// neighbour loads are a row or a plane apart from lane to lane).
__global__ void __launch_bounds__(BLOCK) k_datagen_light(Dim d, const float* __restrict__ val, float* __restrict__ lit) {
	CELL_IJK(d);
	lit[idx] = light_of(d, val, i, j, k);
}

// shadeCell, simpleimage.cpp:218-244
template <bool SURF>
__device__ __forceinline__ void shade(float (&dst)[3], float src, float light, int depthPos, float depthInv) {
	if (SURF) {
		const float t = (float)depthPos * depthInv;
		const double e = (double)t * 0.7 + 0.3;
		const float tint = (float)((double)0.9f * e);          // diffuse[0] *= ..., diffuse[1] *= ...: a double product stored to Real
		const float diffuse[3] = {tint, tint, 0.9f};
		const double a1 = 1. - (double)src;
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const float dl = diffuse[c] * light;
			const float col = 0.1f + dl;
			const float keep = (float)(a1 * (double)dst[c]);   // (1.-alpha) * dst: double scalar times Vec3, rounded per component
			const float add = src * col;
			dst[c] = keep + add;
		}
	} else {
		const float p = depthInv * src;
#pragma unroll
		for (int c = 0; c < 3; c++) dst[c] = dst[c] + p;
	}
}

// mapRange (simpleimage.h:110-117) and writePpm's byte (simpleimage.cpp:49-50)
__device__ __forceinline__ void put_pixel(uint8_t* __restrict__ img, int w, int h, int px, int py, const float (&dst)[3], float f) {
	uint8_t* o = img + ((int64_t)(h - 1 - py) * w + px) * 3;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		float v = dst[c] / f;
		v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
		o[c] = (unsigned char)(255. * (double)v);
	}
}

// VIEW 0: pixel (i, j), marching k, lanes along i.  VIEW 1: pixel (sx + k, j), marching i, lanes along j (each lane walks its own row,
// consuming its cache lines over successive steps).  VIEW 2: pixel (sx + sz + i, k), marching j, lanes along i.
template <int VIEW, bool SURF>
__global__ void __launch_bounds__(BLOCK)
k_datagen_project(Dim d, const float* __restrict__ val, const float* __restrict__ lit, uint8_t* __restrict__ img, int w, int h, float f) {
	const int na = VIEW == 1 ? d.sy : d.sx;                     // the lane axis
	const int nb = VIEW == 0 ? d.sy : d.sz;                     // the other pixel axis
	const int depth = VIEW == 0 ? d.sz : (VIEW == 1 ? d.sx : d.sy);
	const int64_t t = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (t >= (int64_t)na * nb) return;
	const int a = (int)(t % na), b = (int)(t / na);
	const float depthInv = (float)(1. / (double)(float)depth);
	float dst[3] = {0.f, 0.f, 0.f};
	for (int m = 0; m < depth; m++) {
		const int i = VIEW == 1 ? m : a;
		const int j = VIEW == 0 ? b : (VIEW == 1 ? a : m);
		const int k = VIEW == 0 ? m : b;
		const int64_t at = (int64_t)i + (int64_t)d.sx * (j + (int64_t)d.sy * k);
		shade<SURF>(dst, val[at], SURF ? lit[at] : 0.f, m, depthInv);
	}
	if (VIEW == 0) put_pixel(img, w, h, a, b, dst, f);
	if (VIEW == 1) put_pixel(img, w, h, d.sx + b, a, dst, f);
	if (VIEW == 2) put_pixel(img, w, h, d.sx + d.sz + a, b, dst, f);
}

template <int VIEW>
int project_view(const Dim& d, const float* val, const float* lit, uint8_t* img, int w, int h, float f, hipStream_t st) {
	const int64_t n = (int64_t)(VIEW == 1 ? d.sy : d.sx) * (VIEW == 0 ? d.sy : d.sz);
	if (lit)
		hipLaunchKernelGGL((k_datagen_project<VIEW, true>), dim3(nblk(n)), dim3(BLOCK), 0, st, d, val, lit, img, w, h, f);
	else
		hipLaunchKernelGGL((k_datagen_project<VIEW, false>), dim3(nblk(n)), dim3(BLOCK), 0, st, d, val, lit, img, w, h, f);
	MF_LAUNCH_CHECK();
	return 0;
}

// ---- Laplacian and curvature --------------------------------------------------------------------------------------------------------
// LaplaceOp, commonkernels.h:75-80.  KEpsilonGradientDiffusion (turbulence_model.hip, k_ke_grad_diff) has the same three lines inside
// a kernel that also zeroes the border and scales the result; its file belongs to another extension, so the lines are written again.
__global__ void __launch_bounds__(BLOCK) k_datagen_laplacian(Dim d, const float* __restrict__ g, float* __restrict__ lap) {
	CELL_IJK(d);
	if (!INTERIOR(d)) return;
	const double c2 = 2.0 * (double)g[idx];
	float r = (float)(((double)g[idx + 1] - c2) + (double)g[idx - 1]);
	r = (float)((double)r + (((double)g[idx + d.Y] - c2) + (double)g[idx - d.Y]));
	if (d.is3d) r = (float)((double)r + (((double)g[idx + d.Z] - c2) + (double)g[idx - d.Z]));
	lap[idx] = r;
}

// CurvatureOp, commonkernels.h:83-101
__global__ void __launch_bounds__(BLOCK) k_datagen_curvature(Dim d, const float* __restrict__ g, float* __restrict__ curv, float h) {
	CELL_IJK(d);
	if (!INTERIOR(d)) return;
	const int64_t Y = d.Y, Z = d.Z;
	const double oh = (double)(float)(1.0 / (double)h);
	const double c2 = 2.0 * (double)g[idx];
	const float x = (float)((0.5 * (double)(g[idx + 1] - g[idx - 1])) * oh);
	const float y = (float)((0.5 * (double)(g[idx + Y] - g[idx - Y])) * oh);
	const float xx = (float)(((((double)g[idx + 1] - c2) + (double)g[idx - 1]) * oh) * oh);
	const float yy = (float)(((((double)g[idx + Y] - c2) + (double)g[idx - Y]) * oh) * oh);
	const float sxy = ((g[idx + 1 + Y] + g[idx - 1 - Y]) - g[idx - 1 + Y]) - g[idx + 1 - Y];
	const float xy = (float)(((0.25 * (double)sxy) * oh) * oh);
	const float x2 = x * x, y2 = y * y;
	const float n0 = x2 * yy + y2 * xx;
	float cv = (float)((double)n0 - ((2.0 * (double)x) * (double)y) * (double)xy);
	float denom = x2 + y2;
	if (d.is3d) {
		const float z = (float)((0.5 * (double)(g[idx + Z] - g[idx - Z])) * oh);
		const float zz = (float)(((((double)g[idx + Z] - c2) + (double)g[idx - Z]) * oh) * oh);
		const float sxz = ((g[idx + 1 + Z] + g[idx - 1 - Z]) - g[idx - 1 + Z]) - g[idx + 1 - Z];
		const float syz = ((g[idx + Y + Z] + g[idx - Y - Z]) - g[idx + Y - Z]) - g[idx - Y + Z];
		const float xz = (float)(((0.25 * (double)sxz) * oh) * oh);
		const float yz = (float)(((0.25 * (double)syz) * oh) * oh);
		const float z2 = z * z;
		const float n1 = ((x2 * zz + z2 * xx) + y2 * zz) + z2 * yy;
		const float mx = (x * z) * xz + (y * z) * yz;
		cv = (float)((double)cv + ((double)n1 - 2.0 * (double)mx));
		denom = denom + z2;
	}
	const float dm = denom < 1e-6f ? 1e-6f : denom;      // std::max(denom, VECTOR_EPSILON): a NaN denom stays NaN
	curv[idx] = (float)((double)cv / pow((double)dm, 1.5));
}

int check_grid(const char* who, int sx, int sy, int sz) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("%s: not available inside a z-slab window", who);
	return 0;
}

}  // namespace

extern "C" {

int mf_datagen_abi_version(void) { return MF_DATAGEN_ABI_VERSION; }

int mf_datagen_weights(float sigma, int cap, float* w_host, int* mdim_host) {
	if (!w_host || !mdim_host) return fail("mf_datagen_weights: no output");
	Taps t;
	MF_TRY(make_taps("mf_datagen_weights", sigma, cap < MF_DATAGEN_MAX_TAPS ? cap : MF_DATAGEN_MAX_TAPS, &t));
	memcpy(w_host, t.w, sizeof(float) * t.n);
	*mdim_host = t.n;
	return 0;
}

int mf_datagen_blur(int sx, int sy, int sz, int ncomp, const float* src, float* dst, float* tmpA, float* tmpB, float sigma, int* mdim_host,
                    void* stream) {
	MF_TRY(check_grid("mf_datagen_blur", sx, sy, sz));
	if (ncomp != 1 && ncomp != 3) return fail("mf_datagen_blur: %d components", ncomp);
	const Dim d = mkdim(sx, sy, sz);
	if (3 * d.n >= (int64_t)1 << 31) return fail("mf_datagen_blur: grid too large for 32-bit cell indices");
	if (!src || !dst || !tmpA || (d.is3d && !tmpB)) return fail("mf_datagen_blur: missing grid or scratch");
	if (tmpA == src || tmpA == dst || (d.is3d && (tmpB == src || tmpB == dst || tmpB == tmpA))) return fail("mf_datagen_blur: scratch aliases a grid");
	Taps t;
	MF_TRY(make_taps("mf_datagen_blur", sigma, MF_DATAGEN_MAX_TAPS, &t));
	hipStream_t st = (hipStream_t)stream;
	MF_TRY(blur_pass<0>(d, ncomp, src, tmpA, t, st));
	if (d.is3d) {
		MF_TRY(blur_pass<1>(d, ncomp, tmpA, tmpB, t, st));
		MF_TRY(blur_pass<2>(d, ncomp, tmpB, dst, t, st));
	} else {
		MF_TRY(blur_pass<1>(d, ncomp, tmpA, dst, t, st));
	}
	if (mdim_host) *mdim_host = t.n;
	return 0;
}

int mf_datagen_center_of_mass(int sx, int sy, int sz, const float* density, float* out_host, void* stream) {
	MF_TRY(check_grid("mf_datagen_center_of_mass", sx, sy, sz));
	if (!density || !out_host) return fail("mf_datagen_center_of_mass: missing grid or output");
	const Dim d = mkdim(sx, sy, sz);
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	hipStream_t st = (hipStream_t)stream;
	const dim3 grid(blocks_for(d.n, BLOCK * 4, 2048));
	MF_TRY((reduce<SumF64, 4>(d.n, grid, ComTerm{d, density}, ws->partials, ComQuotients{(float*)ws->scalars}, st)));
	return read_scalars(ws, ws->scalars, 3 * sizeof(float), out_host, st);
}

int mf_datagen_project(int sx, int sy, int sz, const float* val, float* light, int shadeMode, float scale, int views, uint8_t* img,
                       void* stream) {
	MF_TRY(check_grid("mf_datagen_project", sx, sy, sz));
	if (!val || !img) return fail("mf_datagen_project: missing grid or image");
	const Dim d = mkdim(sx, sy, sz);
	const bool surf = shadeMode == 1;
	if (surf && (sx < 3 || sy < 3 || (d.is3d && sz < 3)))
		return fail("mf_datagen_project: grid %dx%dx%d is thinner than 3 cells (getGradient would read outside it)", sx, sy, sz);
	if (surf && (!light || light == val)) return fail("mf_datagen_project: surface mode needs a scratch grid for the light");
	const int w = d.is3d ? sx + sz + sx : sx;
	const int h = sx > sy ? (sx > sz ? sx : sz) : (sy > sz ? sy : sz);
	const float f = (float)(1. / (double)scale);
	hipStream_t st = (hipStream_t)stream;
	MF_HIP(hipMemsetAsync(img, 0, (size_t)w * h * 3, st));
	const float* lit = surf ? light : nullptr;
	if (surf) {
		hipLaunchKernelGGL(k_datagen_light, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, val, light);
		MF_LAUNCH_CHECK();
	}
	if (views & 1) MF_TRY(project_view<0>(d, val, lit, img, w, h, f, st));
	if (d.is3d && (views & 2)) MF_TRY(project_view<1>(d, val, lit, img, w, h, f, st));
	if (d.is3d && (views & 4)) MF_TRY(project_view<2>(d, val, lit, img, w, h, f, st));
	return 0;
}

int mf_datagen_laplacian(int sx, int sy, int sz, const float* grid, float* lap, void* stream) {
	MF_TRY(check_grid("mf_datagen_laplacian", sx, sy, sz));
	if (!grid || !lap) return fail("mf_datagen_laplacian: missing grid");
	if (grid == lap) return fail("mf_datagen_laplacian: the output aliases the input");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_datagen_laplacian, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, grid, lap);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_datagen_curvature(int sx, int sy, int sz, const float* grid, float* curv, float h, void* stream) {
	MF_TRY(check_grid("mf_datagen_curvature", sx, sy, sz));
	if (!grid || !curv) return fail("mf_datagen_curvature: missing grid");
	if (grid == curv) return fail("mf_datagen_curvature: the output aliases the input");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_datagen_curvature, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, grid, curv, h);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
