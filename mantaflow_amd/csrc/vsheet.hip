// vsheet.hip -- vortex sheets (include/open/manta_hip_vsheet.h): the channel kernels of VortexSheetMesh and the plugins vorticitySource,
// smoothVorticity, texcoordInflow and meshSmokeInflow, one thread per triangle or node; the per-element bodies are in vsheet_cells.h.
// Reference: source/vortexsheet.{h,cpp}, source/plugin/vortexplugins.cpp:41-166.  Contract: DESIGN.md section 28.
#include "common.h"
#include "vsheet_cells.h"
#include "../../include/open/manta_hip_vsheet.h"
#include "reduce.h"
#include "scan.h"
#include <limits.h>
#include "shape_inside.h"

using namespace mf;
using namespace mf::vsheet;

namespace {

#define VS_LAUNCH(kernel, n, st, ...) hipLaunchKernelGGL(kernel, dim3(nblk(n)), dim3(BLOCK), 0, st, __VA_ARGS__)

int check_mesh(const char* who, int64_t nTris, int64_t tcap, int64_t nNodes, int64_t ncap) {
	if (nTris < 0 || tcap < nTris || nNodes < 0 || ncap < nNodes)
		return fail("%s: %lld triangles / %lld nodes in arrays of stride %lld / %lld", who, (long long)nTris, (long long)nNodes, (long long)tcap, (long long)ncap);
	if (3 * nTris >= (int64_t)1 << 31 || nNodes >= ((int64_t)1 << 31) - 1) return fail("%s: too many triangles or nodes for 32-bit corner numbers", who);
	if (g_slab_gsz > 0) return fail("%s: not available inside a z-slab window", who);
	return 0;
}
int check_shape(const char* who, int kind, const float* params_host, ShapeParams* P) {
	if (kind < 0 || kind > 2) return fail("%s: unknown shape kind %d", who, kind);
	for (int q = 0; q < 12; q++) P->q[q] = params_host[q];
	return 0;
}

__global__ void __launch_bounds__(BLOCK) k_calc_vorticity(MeshView M, const float* __restrict__ circ, float* __restrict__ vort, float* __restrict__ smokeAmount) {
	ITEM_IDX(M.nTris)
	if (tri_outside(M, idx)) return;
	smokeAmount[idx] = 0.f;
	store3(vort, M.tcap, idx, calc_vorticity(M, idx, load3(circ, M.tcap, idx)));
}

// resetTex1 / resetTex2, vortexsheet.cpp:78-86
__global__ void __launch_bounds__(BLOCK) k_reinit_tex(int64_t n, int64_t ncap, const float* __restrict__ pos, V3 off, float* __restrict__ tex1, float* __restrict__ tex2) {
	ITEM_IDX(n)
	const V3 tc = load3(pos, ncap, idx) + off;
	store3(tex1, ncap, idx, tc);
	store3(tex2, ncap, idx, tc);
}

// meshSmokeInflow, vortexplugins.cpp:69-75
__global__ void __launch_bounds__(BLOCK) k_smoke_inflow(MeshView M, int kind, ShapeParams P, float amount, float* __restrict__ smokeAmount) {
	ITEM_IDX(M.nTris)
	if (tri_outside(M, idx)) return;
	const V3 c = face_center(M, idx);
	if (shape_inside(kind, P.q, c.x, c.y, c.z)) smokeAmount[idx] = amount;
}

// KnAcceleration, vortexplugins.cpp:77-80, over the 3 * cells floats of a MAC grid
__global__ void __launch_bounds__(BLOCK) k_acceleration(int64_t n, const float* __restrict__ v1, const float* __restrict__ v0, float idt, float* __restrict__ a) {
	ITEM_IDX(n)
	a[idx] = (v1[idx] - v0[idx]) * idt;
}

// vorticitySource, vortexplugins.cpp:95-117; MACGrid::getInterpolated is interpolMAC (common.h)
__global__ void __launch_bounds__(BLOCK)
k_source(Dim d, const float* __restrict__ accel, MeshView M, V3 gravity, float scale, float maxAmount, float mult, float dt, float dx, float* __restrict__ vort,
         float* __restrict__ normv) {
	ITEM_IDX(M.nTris)
	if (tri_outside(M, idx)) {
		normv[idx] = 0.f;
		return;
	}
	V3 a = {0.f, 0.f, 0.f};
	if (accel) {
		const V3 c = face_center(M, idx);
		interpol_mac(d, accel, c.x, c.y, c.z, a.x, a.y, a.z);
	}
	V3 w = load3(vort, M.tcap, idx);
	normv[idx] = vorticity_source(M, idx, accel != nullptr, a, gravity, scale, maxAmount, mult, dt, dx, w);
	store3(vort, M.tcap, idx, w);
}
struct NormTerm {
	const float* v;
	__device__ __forceinline__ void operator()(int64_t i, double (&acc)[1]) const { acc[0] += (double)v[i]; }
};
struct NormMaxTerm {       // `if (v > maxV) maxV = v` from 0: a NaN never wins
	const float* v;
	__device__ __forceinline__ void operator()(int64_t i, double (&acc)[1]) const { acc[0] = fmax(acc[0], (double)v[i]); }
};

__global__ void __launch_bounds__(BLOCK)
k_smooth_weights(MeshView M, const int32_t* __restrict__ opposite, float mult, float* __restrict__ weights, int32_t* __restrict__ index) {
	ITEM_IDX(3 * M.nTris)
	const int64_t i = idx / 3;
	const int c = (int)(idx % 3);
	const int32_t oc = opposite[idx];
	float w = 0.f;
	int32_t t = 0;
	// a corner table of another triangle list, or a triangle that names no node of the mesh: no neighbour
	if (oc < 3 * M.nTris && !tri_outside(M, i) && (oc < 0 || !tri_outside(M, oc / 3))) smooth_weight(M, opposite, i, c, mult, w, t);
	weights[idx] = w;
	index[idx] = t;
}
// [3][n] <- [3][scap] planes
__global__ void __launch_bounds__(BLOCK) k_gather3(int64_t n, int64_t scap, const float* __restrict__ src, float* __restrict__ dst) {
	ITEM_IDX(n)
	store3(dst, n, idx, load3(src, scap, idx));
}
__global__ void __launch_bounds__(BLOCK)
k_smooth_pass(int64_t n, const float* __restrict__ weights, const int32_t* __restrict__ index, const float* __restrict__ vin, float* __restrict__ vout) {
	ITEM_IDX(n)
	for (int c = 0; c < 3; c++) {
		const int32_t t = index[3 * idx + c];
		if (t < 0 || t >= n) {            // not a table of mf_vsheet_smooth_weights: the triangle keeps its value
			store3(vout, n, idx, load3(vin, n, idx));
			return;
		}
	}
	store3(vout, n, idx, smooth_pass(n, weights, index, vin, idx));
}
// vorticitySmoothed *= alpha, vortexplugins.cpp:165
__global__ void __launch_bounds__(BLOCK) k_scale_out(int64_t n, int64_t tcap, const float* __restrict__ vin, float alpha, float* __restrict__ out) {
	ITEM_IDX(n)
	store3(out, tcap, idx, load3(vin, n, idx) * alpha);
}

// texcoordInflow, vortexplugins.cpp:45-55, in three steps whose cost follows the inside cells, not the grid: (1) one thread per cell
// tests the shape, (2) after an inclusive scan of the marks the inside cells write getCentered at their rank -- the list is in the
// linear cell order, which is FOR_IJK's -- and (3) one wave adds the list serially: 64 values per coalesced load, added in lane order
// into a sum every lane carries.  head as floats: [0..2] = t0 - dt * (sum / (Real)cnt), [3] != 0: an inside cell lies in the last z
// plane (its getCentered reads outside the grid; such a cell is not listed).
__global__ void __launch_bounds__(BLOCK) k_inflow_mark(Dim d, int kind, ShapeParams P, int32_t* __restrict__ mark, float* __restrict__ head) {
	CELL_IJK(d)
	int in = shape_inside(kind, P.q, (float)i + 0.5f, (float)j + 0.5f, (float)k + 0.5f);
	if (in && k >= d.sz - 1) {
		in = 0;
		head[3] = 1.f;
	}
	mark[idx] = in;
}
__global__ void __launch_bounds__(BLOCK) k_inflow_list(Dim d, const float* __restrict__ vel, const int32_t* __restrict__ mark, float* __restrict__ values) {
	CELL_IJK(d)
	const int32_t below = idx ? mark[idx - 1] : 0;
	if (mark[idx] == below) return;
	V3 v;
	get_centered(d, vel, idx, v.x, v.y, v.z);
	store3(values, d.n, below, v);
}
// the value of lane b, b the same in every lane (a scalar read of the register, no trip through the LDS crossbar)
__device__ __forceinline__ float lane_value(float v, int b) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), b)); }
__global__ void __launch_bounds__(64) k_inflow_sum(int64_t n, const int32_t* __restrict__ mark, const float* __restrict__ values, V3 t0, float dt, float* __restrict__ head) {
	const int lane = threadIdx.x;
	const int64_t cnt = mark[n - 1];
	V3 sum = {0.f, 0.f, 0.f};
	for (int64_t base = 0; base < cnt; base += 64) {
		const int64_t q = base + lane;
		const V3 v = q < cnt ? load3(values, n, q) : V3{0.f, 0.f, 0.f};
		const int m = (int)(cnt - base < 64 ? cnt - base : 64);
		if (m == 64) {      // a whole chunk: constant lane numbers
#pragma unroll
			for (int b = 0; b < 64; b++) sum = sum + V3{lane_value(v.x, b), lane_value(v.y, b), lane_value(v.z, b)};
		} else {
			for (int b = 0; b < m; b++) sum = sum + V3{lane_value(v.x, b), lane_value(v.y, b), lane_value(v.z, b)};
		}
	}
	if (lane == 0) {
		const V3 mean = sum / (float)cnt;
		const V3 r = t0 - dt * mean;
		head[0] = r.x;
		head[1] = r.y;
		head[2] = r.z;
	}
}
// vortexplugins.cpp:59-65
__global__ void __launch_bounds__(BLOCK)
k_inflow_apply(int64_t n, int64_t ncap, const float* __restrict__ pos, int kind, ShapeParams P, V3 t0, float* __restrict__ tex1, float* __restrict__ tex2) {
	ITEM_IDX(n)
	const V3 p = load3(pos, ncap, idx);
	if (!shape_inside(kind, P.q, p.x, p.y, p.z)) return;
	const V3 tc = p + t0;
	store3(tex1, ncap, idx, tc);
	store3(tex2, ncap, idx, tc);
}


// ---- VICintegration, vortexplugins.cpp:192-295 ----
// pass A: per triangle the centre, v = (vorticity * area) * fac, wnorm, and the bin of the centre as the sort key
__global__ void __launch_bounds__(BLOCK)
k_spread_tri(Spread S, MeshView M, const float* __restrict__ vort, int64_t nbins, float* __restrict__ tpos, float* __restrict__ tv, float* __restrict__ wnorm,
             uint32_t* __restrict__ key, int32_t* __restrict__ val) {
	ITEM_IDX(M.nTris)
	val[idx] = (int32_t)idx;
	key[idx] = (uint32_t)nbins;
	wnorm[idx] = 0.f;
	if (tri_outside(M, idx)) return;
	const V3 pos = face_center(M, idx);
	const int64_t b = spread_bin(S, pos);
	if (b < 0) return;
	key[idx] = (uint32_t)b;
	store3(tpos, M.nTris, idx, pos);
	store3(tv, M.nTris, idx, (load3(vort, M.tcap, idx) * face_area(M, idx)) * 16.0f);
	wnorm[idx] = spread_wnorm(S, pos);
}
__global__ void __launch_bounds__(BLOCK) k_bin_starts(int64_t n, int64_t nbins, const uint32_t* __restrict__ key, int32_t* __restrict__ start) {
	ITEM_IDX(nbins + 1)
	int64_t lo = 0, hi = n;
	while (lo < hi) {
		const int64_t mid = (lo + hi) >> 1;
		if ((int64_t)key[mid] < idx) lo = mid + 1;
		else hi = mid;
	}
	start[idx] = (int32_t)lo;
}
// pass B: one thread per cell walks the bins whose centres can reach it and takes their triangles in ascending triangle number -- the
// order in which the serial loop adds them.  Within a bin the stable sort has kept the numbers ascending, so the next triangle is the
// smallest lower bound of (last + 1) over the bins.
__global__ void __launch_bounds__(BLOCK)
k_spread_cell(Dim d, Spread S, int64_t nTris, const float* __restrict__ tpos, const float* __restrict__ tv, const float* __restrict__ wnorm,
              const int32_t* __restrict__ start, const int32_t* __restrict__ ids, float* __restrict__ out) {
	CELL_IJK(d)
	V3 acc = {0.f, 0.f, 0.f};
	if (S.flags[idx] & 1) {
		const int m = S.sgi + 1, r = S.sgi + 1;
		const int wx = S.sx + 2 * m, wy = S.sy + 2 * m;
		const int x0 = i + m - r, x1 = i + m + r, y0 = j + m - r, y1 = j + m + r, z0 = k + m - r, z1 = k + m + r;      // inside the widened grid
		int32_t last = -1;
		for (;;) {
			int32_t best = INT_MAX;
			for (int bz = z0; bz <= z1; bz++)
				for (int by = y0; by <= y1; by++) {
					const int64_t row = ((int64_t)bz * wy + by) * wx;
					if (start[row + x0] == start[row + x1 + 1]) continue;
					for (int bx = x0; bx <= x1; bx++) {
						int32_t lo = start[row + bx];
						const int32_t e = start[row + bx + 1];
						int32_t hi = e;
						while (lo < hi) {
							const int32_t mid = (lo + hi) >> 1;
							if (ids[mid] <= last) lo = mid + 1;
							else hi = mid;
						}
						if (lo < e && ids[lo] < best) best = ids[lo];
					}
				}
			if (best == INT_MAX) break;
			spread_add(S, load3(tpos, nTris, best), load3(tv, nTris, best), wnorm[best], i, j, k, acc);
			last = best;
		}
	}
	store3(out, d.n, idx, acc);
}
// CurlOp, commonkernels.h:38-47 (bnd = 1: the border keeps the zero of a fresh grid), 3-D
__global__ void __launch_bounds__(BLOCK) k_curl(Dim d, const float* __restrict__ g, float* __restrict__ dst) {
	CELL_IJK(d)
	V3 v = {0.f, 0.f, 0.f};
	if (INTERIOR(d)) {
		const float *gx = g, *gy = g + d.n, *gz = g + 2 * d.n;
		const int64_t X = 1, Y = d.Y, Z = d.Z;
		v.x = 0.5f * ((gz[idx + Y] - gz[idx - Y]) - (gy[idx + Z] - gy[idx - Z]));
		v.y = 0.5f * ((gx[idx + Z] - gx[idx - Z]) - (gz[idx + X] - gz[idx - X]));
		v.z = 0.5f * ((gy[idx + X] - gy[idx - X]) - (gx[idx + Y] - gx[idx - Y]));
	}
	store3(dst, d.n, idx, v);
}
// GetShiftedComponent (bnd = 1: the border of rhs keeps what it held) / GetComponent, commonkernels.h:104-113
__global__ void __launch_bounds__(BLOCK) k_rhs(Dim d, const float* __restrict__ curl, float* __restrict__ rhs, int c, int shifted) {
	CELL_IJK(d)
	const float* g = curl + (int64_t)c * d.n;
	if (!shifted) {
		rhs[idx] = g[idx];
		return;
	}
	if (!INTERIOR(d)) return;
	const int64_t step = c == 0 ? 1 : (c == 1 ? d.Y : d.Z);
	rhs[idx] = 0.5f * (g[idx] + g[idx - step]);
}
// solution *= scale; SetComponent(vel, solution, c), vortexplugins.cpp:292-293
__global__ void __launch_bounds__(BLOCK) k_set_component(int64_t n, float* __restrict__ vel, float* __restrict__ solution, float scale, int c) {
	ITEM_IDX(n)
	const float v = solution[idx] * scale;
	solution[idx] = v;
	vel[(int64_t)c * n + idx] = v;
}

}  // namespace

extern "C" {

int mf_vsheet_abi_version(void) { return MF_VSHEET_ABI_VERSION; }

int mf_vsheet_calc_vorticity(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, const float* circulation,
                             float* vorticity, float* smokeAmount, void* stream) {
	MF_TRY(check_mesh("VortexSheetMesh::calcVorticity", nTris, tcap, nNodes, ncap));
	if (nTris == 0) return 0;
	const MeshView M = {nTris, tcap, nNodes, ncap, tri, pos, nullptr};
	VS_LAUNCH(k_calc_vorticity, nTris, (hipStream_t)stream, M, circulation, vorticity, smokeAmount);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_vsheet_reinit_tex(int64_t nNodes, int64_t ncap, const float* pos, float ox, float oy, float oz, float* tex1, float* tex2, void* stream) {
	MF_TRY(check_mesh("VortexSheetMesh::reinitTexCoords", 0, 0, nNodes, ncap));
	if (nNodes == 0) return 0;
	VS_LAUNCH(k_reinit_tex, nNodes, (hipStream_t)stream, nNodes, ncap, pos, V3{ox, oy, oz}, tex1, tex2);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_vsheet_smoke_inflow(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, int kind,
                           const float* params_host, float amount, float* smokeAmount, void* stream) {
	MF_TRY(check_mesh("meshSmokeInflow", nTris, tcap, nNodes, ncap));
	ShapeParams P;
	MF_TRY(check_shape("meshSmokeInflow", kind, params_host, &P));
	if (nTris == 0) return 0;
	const MeshView M = {nTris, tcap, nNodes, ncap, tri, pos, nullptr};
	VS_LAUNCH(k_smoke_inflow, nTris, (hipStream_t)stream, M, kind, P, amount, smokeAmount);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_vsheet_acceleration(int sx, int sy, int sz, const float* v1, const float* v0, float idt, float* accel, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("vorticitySource: not available inside a z-slab window");
	const int64_t n = 3 * (int64_t)sx * sy * sz;
	VS_LAUNCH(k_acceleration, n, (hipStream_t)stream, n, v1, v0, idt, accel);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_vsheet_source(int sx, int sy, int sz, const float* accel, int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap,
                     const float* pos, const int32_t* nflags, float gx, float gy, float gz, float scale, float maxAmount, float mult, float dt, float dx,
                     float* vorticity, float* norms, double* stats_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	MF_TRY(check_mesh("vorticitySource", nTris, tcap, nNodes, ncap));
	if (sz < 2) return fail("vorticitySource: 3-D grids only");
	stats_host[0] = stats_host[1] = 0.;
	if (nTris == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	const MeshView M = {nTris, tcap, nNodes, ncap, tri, pos, nflags};
	VS_LAUNCH(k_source, nTris, st, mkdim(sx, sy, sz), accel, M, V3{gx, gy, gz}, scale, maxAmount, mult, dt, dx, vorticity, norms);
	MF_LAUNCH_CHECK();
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const dim3 grid((unsigned)blocks_for(nTris, BLOCK, 1024));
	double* out = (double*)ws->scalars;
	MF_TRY((reduce<MaxF64, 1>(nTris, grid, NormMaxTerm{norms}, ws->partials, Store<double>{out}, st)));
	MF_TRY((reduce<SumF64, 1>(nTris, grid, NormTerm{norms}, ws->partials, Store<double>{out + 1}, st)));
	return read_back(stats_host, out, 2 * sizeof(double), st);
}

int mf_vsheet_smooth_weights(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, const int32_t* opposite,
                             float mult, float* weights, int32_t* index, void* stream) {
	MF_TRY(check_mesh("smoothVorticity", nTris, tcap, nNodes, ncap));
	if (nTris == 0) return 0;
	const MeshView M = {nTris, tcap, nNodes, ncap, tri, pos, nullptr};
	VS_LAUNCH(k_smooth_weights, 3 * nTris, (hipStream_t)stream, M, opposite, mult, weights, index);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_vsheet_smooth_iterate(int64_t nTris, int64_t tcap, const float* weights, const int32_t* index, int iter, float alpha, const float* vorticity,
                             float* smoothed, float* tmp0, float* tmp1, void* stream) {
	MF_TRY(check_mesh("smoothVorticity", nTris, tcap, 0, 0));
	if (nTris == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	float *a = tmp0, *b = tmp1;
	VS_LAUNCH(k_gather3, nTris, st, nTris, tcap, vorticity, a);
	for (int it = 0; it < iter; it++) {
		VS_LAUNCH(k_smooth_pass, nTris, st, nTris, weights, index, (const float*)a, b);
		float* s = a;
		a = b;
		b = s;
	}
	VS_LAUNCH(k_scale_out, nTris, st, nTris, tcap, (const float*)a, alpha, smoothed);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_vsheet_inflow_tmp_bytes(int sx, int sy, int sz, int64_t* bytes_host) {
	MF_TRY(check_dim(sx, sy, sz));
	size_t b = 0;
	(void)inclusive_sum32_bytes((int64_t)sx * sy * sz, &b);      // no device: the entry that uses the scratch fails at its first launch
	*bytes_host = head_ws_bytes(b);
	return 0;
}

int mf_vsheet_inflow_mean(int sx, int sy, int sz, const float* vel, int kind, const float* params_host, float t0x, float t0y, float t0z, float dt,
                          int32_t* mark, float* values, void* tmp, int64_t tmp_bytes, float* out_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("texcoordInflow: not available inside a z-slab window");
	if (sz < 2) return fail("texcoordInflow: 3-D grids only");
	ShapeParams P;
	MF_TRY(check_shape("texcoordInflow", kind, params_host, &P));
	const hipStream_t st = (hipStream_t)stream;
	const Dim d = mkdim(sx, sy, sz);
	int64_t need = 0;
	MF_TRY(mf_vsheet_inflow_tmp_bytes(sx, sy, sz, &need));
	HeadWs h;
	MF_TRY(head_ws_cut("texcoordInflow", tmp, tmp_bytes, need, &h));
	float* head = (float*)h.head;
	MF_HIP(hipMemsetAsync(head, 0, 4 * sizeof(float), st));
	VS_LAUNCH(k_inflow_mark, d.n, st, d, kind, P, mark, head);
	MF_LAUNCH_CHECK();
	MF_TRY(inclusive_sum(h.ws, h.ws_bytes, mark, mark, d.n, st));
	VS_LAUNCH(k_inflow_list, d.n, st, d, vel, (const int32_t*)mark, values);
	hipLaunchKernelGGL(k_inflow_sum, dim3(1), dim3(64), 0, st, d.n, (const int32_t*)mark, (const float*)values, V3{t0x, t0y, t0z}, dt, head);
	MF_LAUNCH_CHECK();
	return read_back(out_host, head, 4 * sizeof(float), st);
}

int mf_vsheet_inflow_apply(int64_t nNodes, int64_t ncap, const float* pos, int kind, const float* params_host, float t0x, float t0y, float t0z,
                           float* tex1, float* tex2, void* stream) {
	MF_TRY(check_mesh("texcoordInflow", 0, 0, nNodes, ncap));
	ShapeParams P;
	MF_TRY(check_shape("texcoordInflow", kind, params_host, &P));
	if (nNodes == 0) return 0;
	VS_LAUNCH(k_inflow_apply, nNodes, (hipStream_t)stream, nNodes, ncap, pos, kind, P, V3{t0x, t0y, t0z}, tex1, tex2);
	MF_LAUNCH_CHECK();
	return 0;
}

static int spread_setup(const char* who, int sx, int sy, int sz, float sigma, const int32_t* flags, Spread* S, int64_t* nbins) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("%s: not available inside a z-slab window", who);
	if (sz < 2) return fail("%s: 3-D grids only", who);
	if (!(sigma > 0.f) || sigma > 16.f) return fail("%s: sigma %g outside (0, 16]", who, (double)sigma);
	S->sx = sx;
	S->sy = sy;
	S->sz = sz;
	S->sgi = (int)ceilf(sigma);
	S->sigma = sigma;
	S->pkfac = (float)(M_PI / (double)sigma);
	S->flags = flags;
	const int m = S->sgi + 1;
	*nbins = (int64_t)(sx + 2 * m) * (sy + 2 * m) * (sz + 2 * m);
	if (*nbins >= ((int64_t)1 << 31) - 2) return fail("%s: grid too large for 32-bit bins", who);
	return 0;
}
struct SpreadTmp {
	uint32_t *k0, *k1;
	int32_t *v0, *v1, *start;
	float *tpos, *tv;
	void* ws;
	size_t ws_bytes;
};
static int64_t spread_need(int64_t nTris, int64_t nbins) {
	const size_t m = (size_t)(nTris > 0 ? nTris : 1);
	size_t b = 0;
	(void)sort_pairs_bytes((int64_t)m, key_bits(nbins), &b);
	return head_ws_bytes(4 * al256(4 * m) + al256(4 * (size_t)(nbins + 1)) + 2 * al256(12 * m) + al256(b));
}
static int spread_cut(void* tmp, int64_t tmp_bytes, int64_t nTris, int64_t nbins, SpreadTmp* t) {
	HeadWs h;
	MF_TRY(head_ws_cut("VICintegration", tmp, tmp_bytes, spread_need(nTris, nbins), &h));
	Cutter cut(h.ws, h.ws_bytes);
	const size_t m = (size_t)(nTris > 0 ? nTris : 1);
	MF_TRY(cut.take(m, &t->k0, &t->k1));
	MF_TRY(cut.take(m, &t->v0, &t->v1));
	MF_TRY(cut.take((size_t)(nbins + 1), &t->start));
	MF_TRY(cut.take(3 * m, &t->tpos, &t->tv));
	t->ws = cut.p;
	t->ws_bytes = cut.left;
	return 0;
}

int mf_vsheet_spread_tmp_bytes(int sx, int sy, int sz, float sigma, int64_t nTris, int64_t* bytes_host) {
	Spread S;
	int64_t nbins;
	MF_TRY(spread_setup("VICintegration", sx, sy, sz, sigma, nullptr, &S, &nbins));
	if (nTris < 0 || nTris >= ((int64_t)1 << 31) - 1) return fail("VICintegration: %lld triangles", (long long)nTris);
	*bytes_host = spread_need(nTris, nbins);
	return 0;
}

int mf_vsheet_spread(int sx, int sy, int sz, const int32_t* flags, int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap,
                     const float* pos, const float* vorticity, float sigma, float* wnorm, float* vort, void* tmp, int64_t tmp_bytes, void* stream) {
	MF_TRY(check_mesh("VICintegration", nTris, tcap, nNodes, ncap));
	Spread S;
	int64_t nbins;
	MF_TRY(spread_setup("VICintegration", sx, sy, sz, sigma, flags, &S, &nbins));
	const hipStream_t st = (hipStream_t)stream;
	const Dim d = mkdim(sx, sy, sz);
	if (nTris == 0) {
		MF_HIP(hipMemsetAsync(vort, 0, 3 * d.n * sizeof(float), st));
		return 0;
	}
	SpreadTmp t;
	MF_TRY(spread_cut(tmp, tmp_bytes, nTris, nbins, &t));
	const MeshView M = {nTris, tcap, nNodes, ncap, tri, pos, nullptr};
	VS_LAUNCH(k_spread_tri, nTris, st, S, M, vorticity, nbins, t.tpos, t.tv, wnorm, t.k0, t.v0);
	MF_LAUNCH_CHECK();
	MF_TRY(sort_pairs(t.ws, t.ws_bytes, t.k0, t.k1, t.v0, t.v1, nTris, key_bits(nbins), st));
	VS_LAUNCH(k_bin_starts, nbins + 1, st, nTris, nbins, (const uint32_t*)t.k1, t.start);
	VS_LAUNCH(k_spread_cell, d.n, st, d, S, nTris, (const float*)t.tpos, (const float*)t.tv, (const float*)wnorm, (const int32_t*)t.start,
	          (const int32_t*)t.v1, vort);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_vsheet_curl(int sx, int sy, int sz, const float* vort, float* curl, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0 || sz < 2) return fail("VICintegration: 3-D whole-domain grids only");
	const Dim d = mkdim(sx, sy, sz);
	VS_LAUNCH(k_curl, d.n, (hipStream_t)stream, d, vort, curl);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_vsheet_rhs(int sx, int sy, int sz, const float* curl, float* rhs, int c, int shifted, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0 || sz < 2) return fail("VICintegration: 3-D whole-domain grids only");
	if (c < 0 || c > 2) return fail("VICintegration: component %d", c);
	const Dim d = mkdim(sx, sy, sz);
	VS_LAUNCH(k_rhs, d.n, (hipStream_t)stream, d, curl, rhs, c, shifted);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_vsheet_set_component(int sx, int sy, int sz, float* vel, float* solution, float scale, int c, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (c < 0 || c > 2) return fail("VICintegration: component %d", c);
	const int64_t n = (int64_t)sx * sy * sz;
	VS_LAUNCH(k_set_component, n, (hipStream_t)stream, n, vel, solution, scale, c);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
