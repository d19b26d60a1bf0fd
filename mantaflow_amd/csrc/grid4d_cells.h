// grid4d_cells.h -- the per-cell bodies of grid4d.hip as __host__ __device__ functions: the kernels call them with one thread per cell
// (lanes along x), and a stand-alone host program (tools/grid4d_host_check.hip) calls the same text in a serial loop, where the host
// sanitizers can watch every index.
//
// fp32 / fp64 map: Real is float; `1.-s1` is a double expression rounded once into the Real; everything else
// of the interpolation is fp32, no contraction (-ffp-contract=off).  The max-diff folds are fp64.
#pragma once
#include "common.h"
#include <math.h>

namespace mf {
namespace grid4d {

#define MF_HD __host__ __device__ __forceinline__

struct Dim4 {
	int sx, sy, sz, st;
	int64_t Y, Z, T, n;   // strides (X == 1) and the cells of one component plane
};
static inline Dim4 mkdim4(int sx, int sy, int sz, int st) {
	Dim4 d;
	d.sx = sx; d.sy = sy; d.sz = sz; d.st = st;
	d.Y = sx;
	d.Z = (int64_t)sx * sy;
	d.T = d.Z * sz;
	d.n = d.T * st;
	return d;
}
struct Cell4 {
	int i, j, k, t;
};
// idx < n < 2^31: 32-bit unsigned divisions are exact
MF_HD Cell4 cell_of(const Dim4& d, int64_t idx) {
	Cell4 c;
	unsigned r = (unsigned)idx;
	unsigned q = r / (unsigned)d.sx;
	c.i = (int)(r - q * (unsigned)d.sx);
	r = q;
	q = r / (unsigned)d.sy;
	c.j = (int)(r - q * (unsigned)d.sy);
	r = q;
	q = r / (unsigned)d.sz;
	c.k = (int)(r - q * (unsigned)d.sz);
	c.t = (int)q;
	return c;
}

// knSetBnd4d, grid4d.cpp:299-307
MF_HD bool is_bound(const Dim4& d, const Cell4& c, int w) {
	return c.i <= w || c.i >= d.sx - 1 - w || c.j <= w || c.j >= d.sy - 1 - w || c.k <= w || c.k >= d.sz - 1 - w || c.t <= w ||
	       c.t >= d.st - 1 - w;
}
// knSetBnd4dNeumann, grid4d.cpp:313-342: the source cell of a boundary cell, -1 for a cell that keeps its value.  Both tests of an
// axis are made in the reference's order, so the upper one wins where both hold.
MF_HD int64_t neumann_source(const Dim4& d, const Cell4& c, int w) {
	bool set = false;
	int si = c.i, sj = c.j, sk = c.k, st = c.t;
	if (c.i <= w) { si = w + 1; set = true; }
	if (c.i >= d.sx - 1 - w) { si = d.sx - 1 - w - 1; set = true; }
	if (c.j <= w) { sj = w + 1; set = true; }
	if (c.j >= d.sy - 1 - w) { sj = d.sy - 1 - w - 1; set = true; }
	if (c.k <= w) { sk = w + 1; set = true; }
	if (c.k >= d.sz - 1 - w) { sk = d.sz - 1 - w - 1; set = true; }
	if (c.t <= w) { st = w + 1; set = true; }
	if (c.t >= d.st - 1 - w) { st = d.st - 1 - w - 1; set = true; }
	if (!set) return -1;
	return (int64_t)si + d.Y * sj + d.Z * sk + d.T * st;
}

// knSetRegion4d, grid4d.cpp:394-400: Vec4 p(i, j, k, t) against start / end in fp32
MF_HD bool in_region(const Cell4& c, const float* start, const float* end) {
	const float p[4] = {(float)c.i, (float)c.j, (float)c.k, (float)c.t};
	for (int q = 0; q < 4; q++)
		if (p[q] < start[q] || p[q] > end[q]) return false;
	return true;
}

// getSliceFrom4d*, grid4d.cpp:407-433: the cell of a dx x dy x dz grid that source cell (i, j, k) goes to, -1 where it has none
MF_HD int64_t slice_target(const Cell4& c, int dx, int dy, int dz) {
	if (c.i >= dx || c.j >= dy || c.k >= dz) return -1;
	return c.i + (int64_t)dx * (c.j + (int64_t)dy * c.k);
}

// one axis of BUILD_INDEX_4D, vector4d.h:396-414.  `(int)p` of a NaN or of a p outside the int range is defined on the device only
// (it saturates, and is 0 for a NaN: with two cells per axis every index stays inside the grid); on the host it is undefined, and the
// host check passes finite positions of grid size only.
MF_HD void axis_index(float pos, int size, int& xi, float& w0, float& w1) {
	const float p = pos - 0.5f;
	xi = (int)p;
	w1 = p - (float)xi;
	w0 = (float)(1. - (double)w1);
	if (p < 0.f) { xi = 0; w0 = 1.f; w1 = 0.f; }
	if (xi >= size - 1) { xi = size - 2; w0 = 0.f; w1 = 1.f; }
}
// interpol4d, vector4d.h:426-442, on one component plane
MF_HD float interpol4d(const Dim4& d, const float* data, float x, float y, float z, float t) {
	int xi, yi, zi, ti;
	float s0, s1, t0, t1, f0, f1, g0, g1;
	axis_index(x, d.sx, xi, s0, s1);
	axis_index(y, d.sy, yi, t0, t1);
	axis_index(z, d.sz, zi, f0, f1);
	axis_index(t, d.st, ti, g0, g1);
	const float* r = data + ((int64_t)xi + d.Y * yi + d.Z * zi + d.T * ti);
	const int64_t Y = d.Y, Z = d.Z, T = d.T;
	const float lo = ((r[0] * t0 + r[Y] * t1) * s0 + (r[1] * t0 + r[1 + Y] * t1) * s1) * f0 +
	                 ((r[Z] * t0 + r[Y + Z] * t1) * s0 + (r[1 + Z] * t0 + r[1 + Y + Z] * t1) * s1) * f1;
	const float hi = ((r[T] * t0 + r[T + Y] * t1) * s0 + (r[T + 1] * t0 + r[T + 1 + Y] * t1) * s1) * f0 +
	                 ((r[T + Z] * t0 + r[T + Y + Z] * t1) * s0 + (r[T + 1 + Z] * t0 + r[T + 1 + Y + Z] * t1) * s1) * f1;
	return lo * g0 + hi * g1;
}
// knInterpol4d, grid4d.cpp:448-453: pos = Vec4(i, j, k, t) * srcFac + offset
MF_HD float interpolate_cell(const Dim4& src, const float* data, const Cell4& c, const float* fac, const float* off) {
	const float x = (float)c.i * fac[0] + off[0], y = (float)c.j * fac[1] + off[1];
	const float z = (float)c.k * fac[2] + off[2], t = (float)c.t * fac[3] + off[3];
	return interpol4d(src, data, x, y, z, t);
}

// normSquare, vectorbase.h:393-395 / vector4d.h:289-291
MF_HD float norm_square(const float* a, int64_t n, int64_t idx, int ncomp) {   // n: the distance of the component planes
	float s = a[idx] * a[idx] + a[n + idx] * a[n + idx] + a[2 * n + idx] * a[2 * n + idx];
	if (ncomp == 4) s = s + a[3 * n + idx] * a[3 * n + idx];
	return s;
}
// one cell of grid4dMaxDiff / Int / Vec3 / Vec4, grid4d.cpp:352-391
MF_HD double cell_diff(const void* a, const void* b, int64_t n, int64_t idx, int ncomp, int isInt) {
	if (isInt) return fabs((double)((const int32_t*)a)[idx] - (double)((const int32_t*)b)[idx]);
	const float *fa = (const float*)a, *fb = (const float*)b;
	if (ncomp == 1) return (double)fabsf(fa[idx] - fb[idx]);
	double s = 0.;
	for (int c = 0; c < ncomp; c++) s += fabs((double)fa[c * n + idx] - (double)fb[c * n + idx]);
	return s;
}

MF_HD int32_t clamp_i(int32_t v, int32_t lo, int32_t hi) {
	if (v < lo) return lo;
	if (v > hi) return hi;
	return v;
}
// int arithmetic wraps (unsigned arithmetic has no undefined overflow; the words are those of gcc's wrapping int code)
MF_HD int32_t add_i(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
MF_HD int32_t sub_i(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
MF_HD int32_t mul_i(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }

// safeDivide<int>, general.h:149
MF_HD int32_t safe_div_i(int32_t a, int32_t b) {
	if (!b) return a;
	if (b == -1) return sub_i(0, a);
	return a / b;
}

// ---- particle data, particle.cpp:445-459, 565-567 ----
// std::max(v, x) and std::min(v, x) as the library writes them: the first argument is returned unless the comparison holds
template <class T> MF_HD T clamp_side(int side, T v, T x) { return side == 0 ? (v < x ? x : v) : (x < v ? x : v); }

// norm(Vec3), vectorbase.h:385-389: VECTOR_EPSILON * VECTOR_EPSILON is a float product, `l - 1.` a double difference
MF_HD float norm3(float x, float y, float z) {
	const float l = x * x + y * y + z * z;
	const float eps2 = 1e-6f * 1e-6f;
	if (l <= eps2) return 0.f;
	return fabs((double)l - 1.) < (double)eps2 ? 1.f : sqrtf(l);
}
// the term slot idx adds to KnPtsSum (what 0, component c), KnPtsSumSquare (1) or KnPtsSumMagnitude (2), as the double it is added as
MF_HD double sum_term(int what, int isInt, int ncomp, int c, const void* a, int64_t stride, int64_t idx) {
	if (isInt) {
		const int32_t v = ((const int32_t*)a)[idx];
		if (what == 0) return (double)v;
		if (what == 1) return (double)(float)mul_i(v, v);
		return (double)(float)(v < 0 ? sub_i(0, v) : v);
	}
	const float* f = (const float*)a;
	if (what == 0) return (double)f[c * stride + idx];
	if (ncomp == 1) return what == 1 ? (double)(f[idx] * f[idx]) : (double)fabsf(f[idx]);
	const float x = f[idx], y = f[stride + idx], z = f[2 * stride + idx];
	return what == 1 ? (double)(x * x + y * y + z * z) : (double)norm3(x, y, z);
}

// ---- checkSymmetry / checkSymmetryVec3, initplugins.cpp:189-269, one sweep of the serial loop restated as two passes.  A cell and its
// mirror differ in coordinate `axis` only, so the mirror with the smaller coordinate comes first in the loop: a "first-half" cell
// (coordinate < s/2, or the centre line of the MAC form) reads a mirror no sweep writes, and is the only kind that is written; every
// other cell reads a mirror that the sweep has already symmetrised.  Pass 0 does the first-half cells, pass 1 the others.
struct Sym {
	int axis, bound, symmetrize;
	int mac;      // 1: the normal component of the MAC form (s = size + 1, sign flipped, centre line)
};
MF_HD bool sym_in_bounds(const Dim& d, int i, int j, int k, int b) {
	bool ret = i >= b && j >= b && i < d.sx - b && j < d.sy - b;
	if (d.is3d) ret = ret && (k >= b && k < d.sz - b);
	else ret = ret && k == 0;
	return ret;
}
// a: the component plane that is compared; err may be null.  add: `err +=` (the MAC form) rather than `err =`.
MF_HD void sym_cell(const Dim& d, int i, int j, int k, int pass, const Sym& S, float* a, float* err, bool add) {
	const int size = S.axis == 0 ? d.sx : S.axis == 1 ? d.sy : d.sz;
	const int s = size + (S.mac ? 1 : 0);
	const int me = S.axis == 0 ? i : S.axis == 1 ? j : k;
	const int mir = s - 1 - me;
	if (mir >= size) return;
	const bool centre = S.mac && mir == me;
	const bool first = centre || me < s / 2;
	if (first != (pass == 0)) return;
	const int mi = S.axis == 0 ? mir : i, mj = S.axis == 1 ? mir : j, mk = S.axis == 2 ? mir : k;
	if (S.bound > 0 && (!sym_in_bounds(d, i, j, k, S.bound) || !sym_in_bounds(d, mi, mj, mk, S.bound))) return;
	const int64_t idx = i + d.sx * (int64_t)(j + (int64_t)d.sy * k), mdx = mi + d.sx * (int64_t)(mj + (int64_t)d.sy * mk);
	double e;
	if (centre) e = fabs((double)a[idx]);
	else if (S.mac) e = fabs((double)a[idx] - ((double)a[mdx] * -1.));
	else e = fabs((double)(a[idx] - a[mdx]));
	if (err) err[idx] = add ? (float)((double)err[idx] + e) : (float)e;
	if (S.symmetrize) {
		if (centre) a[idx] = 0.f;
		else if (me < s / 2) a[idx] = S.mac ? -a[mdx] : a[mdx];
	}
}

}  // namespace grid4d
}  // namespace mf
