// grid4d.hip -- the 4-D grids (include/open/manta_hip_grid4d.h): one thread per cell with lanes along x, components of the vector types
// along blockIdx.y; the per-cell bodies are in grid4d_cells.h.
// Reference: grid4d.h, grid4d.cpp, util/vector4d.h:393-442.
#include "grid4d_cells.h"
#include "reduce.h"
#include <type_traits>
#include "wavelet_noise_vec.h"
#include "../../include/open/manta_hip_grid4d.h"

using namespace mf;
using namespace mf::grid4d;

namespace {

struct F4 {
	float v[4];
};
struct I4 {
	int32_t v[4];
};

__global__ void __launch_bounds__(BLOCK) k_vec_const(int op, int64_t n, float* __restrict__ me, F4 v) {
	ITEM_IDX(n)
	const int c = blockIdx.y;
	float* p = me + c * n + idx;
	if (op == 0) *p = v.v[c];
	else if (op == 1) *p += v.v[c];
	else *p *= v.v[c];
}

// me may be other (a.addScaled(a, f)): no __restrict__
__global__ void __launch_bounds__(BLOCK) k_vec_scaled_add(int64_t n, float* me, const float* other, F4 f) {
	ITEM_IDX(n)
	const int c = blockIdx.y;
	me[c * n + idx] += f.v[c] * other[c * n + idx];
}

__global__ void __launch_bounds__(BLOCK) k_int_const(int op, int64_t n, int32_t* __restrict__ me, int32_t v) {
	ITEM_IDX(n)
	me[idx] = op == 1 ? add_i(me[idx], v) : mul_i(me[idx], v);
}

// me may be other (a.add(a)): no __restrict__
__global__ void __launch_bounds__(BLOCK) k_int_binary(int op, int64_t n, int32_t* me, const int32_t* other, int32_t factor) {
	ITEM_IDX(n)
	const int32_t a = me[idx], b = other[idx];
	me[idx] = op == 0 ? add_i(a, b) : op == 1 ? sub_i(a, b) : op == 2 ? mul_i(a, b) : op == 3 ? add_i(a, mul_i(factor, b)) : safe_div_i(a, b);
}

__global__ void __launch_bounds__(BLOCK) k_int_clamp(int64_t n, int32_t* __restrict__ me, int32_t lo, int32_t hi) {
	ITEM_IDX(n)
	me[idx] = clamp_i(me[idx], lo, hi);
}

// ---- the terms of the reductions (reduce.h) ----
struct IntMinMaxTerm {
	const int32_t* a;
	__device__ __forceinline__ void operator()(int64_t idx, Pair<int32_t> (&acc)[1]) const { MinMaxI32::fold(acc[0], a[idx]); }
};
struct NormMinMaxTerm {
	int ncomp;
	int64_t stride;
	const float* a;
	__device__ __forceinline__ void operator()(int64_t idx, Pair<float> (&acc)[1]) const { MinMaxF32::fold(acc[0], norm_square(a, stride, idx, ncomp)); }
};
struct MaxDiffTerm {
	int ncomp, isInt;
	int64_t n;
	const void *a, *b;
	__device__ __forceinline__ void operator()(int64_t idx, double (&acc)[1]) const { MaxF64::fold(acc[0], cell_diff(a, b, n, idx, ncomp, isInt)); }
};

// ---- boundaries, region, slices, components ----
__global__ void __launch_bounds__(BLOCK) k_set_bound(Dim4 d, int32_t* __restrict__ grid, I4 v, int w) {
	ITEM_IDX(d.n)
	if (is_bound(d, cell_of(d, idx), w)) grid[blockIdx.y * d.n + idx] = v.v[blockIdx.y];
}
// in place: the source of a boundary cell is no boundary cell (the entry refuses axes below 2w+3), so nothing read here is written here
__global__ void __launch_bounds__(BLOCK) k_set_bound_neumann(Dim4 d, int32_t* grid, int w) {
	ITEM_IDX(d.n)
	const int64_t src = neumann_source(d, cell_of(d, idx), w);
	if (src >= 0) grid[blockIdx.y * d.n + idx] = grid[blockIdx.y * d.n + src];
}
__global__ void __launch_bounds__(BLOCK) k_set_region(Dim4 d, float* __restrict__ grid, F4 start, F4 end, F4 v) {
	ITEM_IDX(d.n)
	if (in_region(cell_of(d, idx), start.v, end.v)) grid[blockIdx.y * d.n + idx] = v.v[blockIdx.y];
}
__global__ void __launch_bounds__(BLOCK) k_copy_plane(int64_t n, const float* __restrict__ src, float* __restrict__ dst) {
	ITEM_IDX(n)
	dst[idx] = src[idx];
}
// one thread per cell (i, j, k) of the source's 3-D slab; blockIdx.y is the component of the Vec4 form
__global__ void __launch_bounds__(BLOCK)
k_get_slice(Dim4 d, const float* __restrict__ src, int srct, int dx, int dy, int dz, float* __restrict__ dst, float* __restrict__ dstt) {
	ITEM_IDX(d.T)
	const int64_t di = slice_target(cell_of(d, idx), dx, dy, dz);
	if (di < 0) return;
	const int comp = blockIdx.y;
	const int64_t dn = (int64_t)dx * dy * dz;
	const float val = src[comp * d.n + d.T * srct + idx];
	if (comp < 3) dst[comp * dn + di] = val;
	else if (dstt) dstt[di] = val;
}

__global__ void __launch_bounds__(BLOCK) k_interpolate(Dim4 td, float* __restrict__ target, Dim4 sd, const float* __restrict__ source, F4 fac, F4 off) {
	ITEM_IDX(td.n)
	target[blockIdx.y * td.n + idx] = interpolate_cell(sd, source + blockIdx.y * sd.n, cell_of(td, idx), fac.v, off.v);
}

// ---- particle data ----
struct I3 {
	int32_t v[3];
};
__global__ void __launch_bounds__(BLOCK) k_pdata_set_flag(int64_t n, int64_t stride, int32_t* __restrict__ me, I3 w, const int32_t* __restrict__ t, int itype) {
	ITEM_IDX(n)
	if (t[idx] & itype) me[blockIdx.y * stride + idx] = w.v[blockIdx.y];
}
__global__ void __launch_bounds__(BLOCK) k_pdata_clamp_side(int side, int isInt, int64_t n, int64_t stride, int32_t* __restrict__ me, int32_t v) {
	ITEM_IDX(n)
	int32_t* p = me + blockIdx.y * stride + idx;
	if (isInt) *p = clamp_side<int32_t>(side, v, *p);
	else *(float*)p = clamp_side<float>(side, __int_as_float(v), *(float*)p);
}
// one term of component blockIdx.y; EXACT: the int sum (what == 0 of an int array), folded as 64-bit integers, which is exact whatever
// the order (as doubles the two halves of a large sum would lose bits)
template <bool EXACT>
struct PdataSumTerm {
	int what, isInt, ncomp;
	int64_t stride;
	const void* a;
	const int32_t* t;
	int itype;
	__device__ __forceinline__ void operator()(int64_t idx, std::conditional_t<EXACT, long long, double> (&acc)[1]) const {
		if (what == 0 && t && !(t[idx] & itype)) return;
		if (EXACT) acc[0] += ((const int32_t*)a)[idx];
		else acc[0] += sum_term(what, isInt, ncomp, blockIdx.y, a, stride, idx);
	}
};
// out[c] = the fp32 of the folded partials of component c, or the wrapped int32 of the exact sum
struct StorePdataSum {
	int32_t* out;
	__device__ __forceinline__ void operator()(const double (&acc)[1]) const { out[blockIdx.x] = __float_as_int((float)acc[0]); }
	__device__ __forceinline__ void operator()(const long long (&acc)[1]) const { out[blockIdx.x] = (int32_t)(uint32_t)(unsigned long long)acc[0]; }
};

// the grid of the reductions over n items
dim3 grid_for(int64_t n) { return dim3(blocks_for(n, BLOCK * 8, 1024)); }

int check_pdata(const char* who, int64_t n, int64_t stride, int ncomp) {
	if (n < 0 || n >= (int64_t)1 << 31 || stride < n) return fail("%s: invalid size %lld / stride %lld", who, (long long)n, (long long)stride);
	if (ncomp != 1 && ncomp != 3) return fail("%s: invalid ncomp %d", who, ncomp);
	return 0;
}

// one thread per slot; the tile index is masked to 128^3, so any position reads inside the tile
__global__ void __launch_bounds__(BLOCK)
k_pdata_set_noise(int kind, int64_t n, int64_t stride, void* __restrict__ pd, int64_t pstride, const float* __restrict__ pos,
                  const float* __restrict__ tile, NoiseParams P, float scale) {
	ITEM_IDX(n)
	const float x = pos[idx], y = pos[pstride + idx], z = pos[2 * pstride + idx];
	if (kind == 2) {
		float v[3];
		noise_evaluate_vec(P, tile, x, y, z, 0, v);
		for (int c = 0; c < 3; c++) ((float*)pd)[c * stride + idx] = v[c] * scale;
	} else {
		const float v = noise_evaluate(P, tile, x, y, z) * scale;
		if (kind == 0) ((float*)pd)[idx] = v;
		else ((int32_t*)pd)[idx] = (int32_t)v;
	}
}

__global__ void __launch_bounds__(BLOCK) k_check_symmetry(Dim d, int pass, Sym S, float* a, float* err, int add) {
	CELL_IJK(d)
	sym_cell(d, i, j, k, pass, S, a, err, add != 0);
}
__global__ void __launch_bounds__(BLOCK) k_init_grid_with_pos(Dim d, float* __restrict__ grid) {
	CELL_IJK(d)
	grid[idx] = norm3((float)i, (float)j, (float)k);
}

int check_dim4(const char* who, int sx, int sy, int sz, int st) {
	if (sx < 1 || sy < 1 || sz < 1 || st < 1) return fail("%s: invalid grid size %dx%dx%dx%d", who, sx, sy, sz, st);
	if ((double)sx * sy * sz * st >= 2147483648.) return fail("%s: grid too large for 32-bit cell indices", who);
	return 0;
}
int check_n(const char* who, int64_t n) {
	if (n < 1 || n >= (int64_t)1 << 31) return fail("%s: invalid size %lld", who, (long long)n);
	return 0;
}
int check_ncomp(const char* who, int ncomp, bool one) {
	if (!(ncomp == 3 || ncomp == 4 || (one && ncomp == 1))) return fail("%s: invalid ncomp %d", who, ncomp);
	return 0;
}

}  // namespace

extern "C" {

int mf_grid4d_abi_version(void) { return MF_GRID4D_ABI_VERSION; }

int mf_grid4d_vec_const(int op, int ncomp, int64_t n, float* me, float vx, float vy, float vz, float vt, void* stream) {
	MF_TRY(check_n("mf_grid4d_vec_const", n));
	MF_TRY(check_ncomp("mf_grid4d_vec_const", ncomp, false));
	if (op < 0 || op > 2) return fail("mf_grid4d_vec_const: invalid op %d", op);
	const F4 v = {{vx, vy, vz, vt}};
	hipLaunchKernelGGL(k_vec_const, dim3(nblk(n), ncomp), dim3(BLOCK), 0, (hipStream_t)stream, op, n, me, v);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_vec_scaled_add(int ncomp, int64_t n, float* me, const float* other, float fx, float fy, float fz, float ft, void* stream) {
	MF_TRY(check_n("mf_grid4d_vec_scaled_add", n));
	MF_TRY(check_ncomp("mf_grid4d_vec_scaled_add", ncomp, false));
	const F4 f = {{fx, fy, fz, ft}};
	hipLaunchKernelGGL(k_vec_scaled_add, dim3(nblk(n), ncomp), dim3(BLOCK), 0, (hipStream_t)stream, n, me, other, f);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_int_const(int op, int64_t n, int32_t* me, int32_t v, void* stream) {
	MF_TRY(check_n("mf_grid4d_int_const", n));
	if (op < 1 || op > 2) return fail("mf_grid4d_int_const: invalid op %d", op);
	hipLaunchKernelGGL(k_int_const, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, op, n, me, v);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_int_binary(int op, int64_t n, int32_t* me, const int32_t* other, int32_t factor, void* stream) {
	MF_TRY(check_n("mf_grid4d_int_binary", n));
	if (op < 0 || op > 4) return fail("mf_grid4d_int_binary: invalid op %d", op);
	hipLaunchKernelGGL(k_int_binary, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, op, n, me, other, factor);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_int_clamp(int64_t n, int32_t* me, int32_t lo, int32_t hi, void* stream) {
	MF_TRY(check_n("mf_grid4d_int_clamp", n));
	hipLaunchKernelGGL(k_int_clamp, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, me, lo, hi);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_int_min_max(int64_t n, const int32_t* a, int32_t* min_host, int32_t* max_host, void* stream) {
	MF_TRY(check_n("mf_grid4d_int_min_max", n));
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const hipStream_t st = (hipStream_t)stream;
	Pair<int32_t>*part = (Pair<int32_t>*)ws->fpartials, *out = (Pair<int32_t>*)ws->scalars, r;
	MF_TRY((reduce<MinMaxI32, 1>(n, grid_for(n), IntMinMaxTerm{a}, part, Store<Pair<int32_t>>{out}, st)));
	MF_TRY(read_scalars(ws, out, sizeof(r), &r, st));
	*min_host = r.lo;
	*max_host = r.hi;
	return 0;
}

int mf_grid4d_norm_min_max(int ncomp, int64_t n, int64_t stride, const float* a, float* min_host, float* max_host, void* stream) {
	MF_TRY(check_n("mf_grid4d_norm_min_max", n));
	if (stride < n) return fail("mf_grid4d_norm_min_max: stride %lld below n %lld", (long long)stride, (long long)n);
	MF_TRY(check_ncomp("mf_grid4d_norm_min_max", ncomp, false));
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const hipStream_t st = (hipStream_t)stream;
	Pair<float>*part = (Pair<float>*)ws->fpartials, *out = (Pair<float>*)ws->scalars, r;
	MF_TRY((reduce<MinMaxF32, 1>(n, grid_for(n), NormMinMaxTerm{ncomp, stride, a}, part, Store<Pair<float>>{out}, st)));
	MF_TRY(read_scalars(ws, out, sizeof(r), &r, st));
	*min_host = r.lo;
	*max_host = r.hi;
	return 0;
}

int mf_grid4d_max_diff(int ncomp, int isInt, int64_t n, const void* a, const void* b, double* result_host, void* stream) {
	MF_TRY(check_n("mf_grid4d_max_diff", n));
	MF_TRY(check_ncomp("mf_grid4d_max_diff", ncomp, true));
	if (isInt && ncomp != 1) return fail("mf_grid4d_max_diff: int grids have one component");
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const hipStream_t st = (hipStream_t)stream;
	MF_TRY((reduce<MaxF64, 1>(n, grid_for(n), MaxDiffTerm{ncomp, isInt, n, a, b}, ws->partials, Store<double>{(double*)ws->scalars}, st)));
	return read_scalars(ws, ws->scalars, sizeof(double), result_host, st);
}

int mf_grid4d_set_bound(int sx, int sy, int sz, int st, void* grid, int ncomp, int32_t v0, int32_t v1, int32_t v2, int32_t v3, int w,
                        void* stream) {
	MF_TRY(check_dim4("mf_grid4d_set_bound", sx, sy, sz, st));
	MF_TRY(check_ncomp("mf_grid4d_set_bound", ncomp, true));
	const Dim4 d = mkdim4(sx, sy, sz, st);
	const I4 v = {{v0, v1, v2, v3}};
	hipLaunchKernelGGL(k_set_bound, dim3(nblk(d.n), ncomp), dim3(BLOCK), 0, (hipStream_t)stream, d, (int32_t*)grid, v, w);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_set_bound_neumann(int sx, int sy, int sz, int st, void* grid, int ncomp, int w, void* stream) {
	MF_TRY(check_dim4("mf_grid4d_set_bound_neumann", sx, sy, sz, st));
	MF_TRY(check_ncomp("mf_grid4d_set_bound_neumann", ncomp, true));
	const int lo = sx < sy ? (sx < sz ? (sx < st ? sx : st) : (sz < st ? sz : st)) : (sy < sz ? (sy < st ? sy : st) : (sz < st ? sz : st));
	if (w < 0 || w > (1 << 20) || lo < 2 * w + 3)
		return fail("mf_grid4d_set_bound_neumann: grid %dx%dx%dx%d too small for boundaryWidth %d", sx, sy, sz, st, w);
	const Dim4 d = mkdim4(sx, sy, sz, st);
	hipLaunchKernelGGL(k_set_bound_neumann, dim3(nblk(d.n), ncomp), dim3(BLOCK), 0, (hipStream_t)stream, d, (int32_t*)grid, w);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_get_comp(int64_t n, const float* src4, float* dst, int c, void* stream) {
	MF_TRY(check_n("mf_grid4d_get_comp", n));
	if (c < 0 || c > 3) return fail("mf_grid4d_get_comp: invalid component %d", c);
	hipLaunchKernelGGL(k_copy_plane, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, src4 + c * n, dst);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_set_comp(int64_t n, const float* src, float* dst4, int c, void* stream) {
	MF_TRY(check_n("mf_grid4d_set_comp", n));
	if (c < 0 || c > 3) return fail("mf_grid4d_set_comp: invalid component %d", c);
	hipLaunchKernelGGL(k_copy_plane, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, src, dst4 + c * n);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_set_region(int sx, int sy, int sz, int st, float* grid, int ncomp, float s0, float s1, float s2, float s3, float e0,
                         float e1, float e2, float e3, float v0, float v1, float v2, float v3, void* stream) {
	MF_TRY(check_dim4("mf_grid4d_set_region", sx, sy, sz, st));
	if (ncomp != 1 && ncomp != 4) return fail("mf_grid4d_set_region: invalid ncomp %d", ncomp);
	const Dim4 d = mkdim4(sx, sy, sz, st);
	const F4 s = {{s0, s1, s2, s3}}, e = {{e0, e1, e2, e3}}, v = {{v0, v1, v2, v3}};
	hipLaunchKernelGGL(k_set_region, dim3(nblk(d.n), ncomp), dim3(BLOCK), 0, (hipStream_t)stream, d, grid, s, e, v);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_get_slice(int sx, int sy, int sz, int st, const float* src, int ncomp, int srct, int dx, int dy, int dz, float* dst,
                        float* dstt, void* stream) {
	MF_TRY(check_dim4("mf_grid4d_get_slice", sx, sy, sz, st));
	if (ncomp != 1 && ncomp != 4) return fail("mf_grid4d_get_slice: invalid ncomp %d", ncomp);
	if (dx < 1 || dy < 1 || dz < 1 || (double)dx * dy * dz >= 2147483648.) return fail("mf_grid4d_get_slice: invalid target size %dx%dx%d", dx, dy, dz);
	if (srct < 0 || srct >= st) return 0;
	const Dim4 d = mkdim4(sx, sy, sz, st);
	hipLaunchKernelGGL(k_get_slice, dim3(nblk(d.T), ncomp), dim3(BLOCK), 0, (hipStream_t)stream, d, src, srct, dx, dy, dz, dst, dstt);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_interpolate(int tx, int ty, int tz, int tt, float* target, int sx, int sy, int sz, int st, const float* source, int ncomp,
                          float f0, float f1, float f2, float f3, float o0, float o1, float o2, float o3, void* stream) {
	MF_TRY(check_dim4("mf_grid4d_interpolate", tx, ty, tz, tt));
	MF_TRY(check_dim4("mf_grid4d_interpolate", sx, sy, sz, st));
	if (ncomp != 1 && ncomp != 4) return fail("mf_grid4d_interpolate: invalid ncomp %d", ncomp);
	if (sx < 2 || sy < 2 || sz < 2 || st < 2) return fail("mf_grid4d_interpolate: every axis of the source needs 2 cells, got %dx%dx%dx%d", sx, sy, sz, st);
	if (target == source) return fail("mf_grid4d_interpolate: target must not alias source");
	const Dim4 td = mkdim4(tx, ty, tz, tt), sd = mkdim4(sx, sy, sz, st);
	const F4 fac = {{f0, f1, f2, f3}}, off = {{o0, o1, o2, o3}};
	hipLaunchKernelGGL(k_interpolate, dim3(nblk(td.n), ncomp), dim3(BLOCK), 0, (hipStream_t)stream, td, target, sd, source, fac, off);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_pdata_set_flag(int64_t n, int64_t stride, int ncomp, void* me, int32_t w0, int32_t w1, int32_t w2, const int32_t* t,
                             int itype, void* stream) {
	MF_TRY(check_pdata("mf_grid4d_pdata_set_flag", n, stride, ncomp));
	if (n == 0) return 0;
	const I3 w = {{w0, w1, w2}};
	hipLaunchKernelGGL(k_pdata_set_flag, dim3(nblk(n), ncomp), dim3(BLOCK), 0, (hipStream_t)stream, n, stride, (int32_t*)me, w, t, itype);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_pdata_clamp_side(int side, int isInt, int64_t n, int64_t stride, int ncomp, void* me, int32_t v, void* stream) {
	MF_TRY(check_pdata("mf_grid4d_pdata_clamp_side", n, stride, ncomp));
	if (side < 0 || side > 1 || (isInt && ncomp != 1)) return fail("mf_grid4d_pdata_clamp_side: invalid side %d / isInt %d", side, isInt);
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_pdata_clamp_side, dim3(nblk(n), ncomp), dim3(BLOCK), 0, (hipStream_t)stream, side, isInt, n, stride, (int32_t*)me, v);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_pdata_sum(int what, int isInt, int ncomp, int64_t n, int64_t stride, const void* a, const int32_t* t, int itype,
                        void* result_host, void* stream) {
	MF_TRY(check_pdata("mf_grid4d_pdata_sum", n, stride, ncomp));
	if (what < 0 || what > 2 || (isInt && ncomp != 1)) return fail("mf_grid4d_pdata_sum: invalid what %d / isInt %d", what, isInt);
	const int nres = what == 0 ? ncomp : 1;
	if (n == 0) {
		memset(result_host, 0, 4 * nres);
		return 0;
	}
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const hipStream_t st = (hipStream_t)stream;
	const dim3 grid(grid_for(n).x, nres);
	const StorePdataSum out = {(int32_t*)ws->scalars};
	if (isInt && what == 0)
		MF_TRY((reduce<SumI64, 1>(n, grid, PdataSumTerm<true>{what, isInt, ncomp, stride, a, t, itype}, (long long*)ws->partials, out, st)));
	else
		MF_TRY((reduce<SumF64, 1>(n, grid, PdataSumTerm<false>{what, isInt, ncomp, stride, a, t, itype}, ws->partials, out, st)));
	return read_scalars(ws, ws->scalars, 4 * nres, result_host, st);
}

int mf_grid4d_pdata_set_noise(int kind, int64_t n, int64_t stride, void* pd, int64_t pstride, const float* pos, const float* tile,
                              const float* params, float scale, void* stream) {
	MF_TRY(check_pdata("mf_grid4d_pdata_set_noise", n, stride, kind == 2 ? 3 : 1));
	if (kind < 0 || kind > 2 || pstride < n) return fail("mf_grid4d_pdata_set_noise: invalid kind %d / position stride %lld", kind, (long long)pstride);
	if (n == 0) return 0;
	const NoiseParams P = noise_params_vec(params);
	hipLaunchKernelGGL(k_pdata_set_noise, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, kind, n, stride, pd, pstride, pos, tile, P, scale);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_check_symmetry(int sx, int sy, int sz, float* a, int mac, float* err, int symmetrize, int axis, int bound, int disable,
                             void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (axis < 0 || axis > 2) return fail("mf_grid4d_check_symmetry: invalid axis %d", axis);
	const hipStream_t st = (hipStream_t)stream;
	Dim d = mkdim(sx, sy, sz);
	d.zoff = 0;
	d.gsz = sz;
	if (mac && err) MF_HIP(hipMemsetAsync(err, 0, sizeof(float) * d.n, st));
	for (int q = 0; q < (mac ? 3 : 1); q++) {
		if (mac && (disable >> q & 1)) continue;
		const int comp = mac ? (axis + q) % 3 : 0;
		const Sym S = {axis, bound, symmetrize, mac && q == 0};
		for (int pass = 0; pass < 2; pass++)
			hipLaunchKernelGGL(k_check_symmetry, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, pass, S, a + comp * d.n, err, mac);
	}
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_grid4d_init_grid_with_pos(int sx, int sy, int sz, float* grid, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_init_grid_with_pos, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, grid);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
