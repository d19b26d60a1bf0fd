// vsheet_cells.h -- the per-triangle, per-node and per-cell bodies of vsheet.hip as __host__ __device__ functions: the kernels call them
// with one thread per element, and a stand-alone host program (tools/vsheet_host_check.hip) calls the same text in serial loops, where
// the host sanitizers can watch every index.  Reference: source/mesh.h:207-215, source/vortexsheet.cpp, source/plugin/vortexplugins.cpp.
// Contract and fp32 / fp64 map: DESIGN.md section 28.  Built with -ffp-contract=off: every product and sum rounds on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace mf {
namespace vsheet {

#define MF_VS_HD __host__ __device__ __forceinline__

struct V3 {
	float x, y, z;
};
MF_VS_HD V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
MF_VS_HD V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
MF_VS_HD V3 operator*(float s, V3 v) { return {s * v.x, s * v.y, s * v.z}; }      // vectorbase.h:281-284
MF_VS_HD V3 operator*(V3 v, float s) { return {v.x * s, v.y * s, v.z * s}; }      // vectorbase.h:276-279
MF_VS_HD V3 operator/(V3 v, float s) { return {v.x / s, v.y / s, v.z / s}; }      // vectorbase.h:292-295
// cross, vectorbase.h:362-368
MF_VS_HD V3 cross(V3 t, V3 v) { return {(t.y * v.z) - (t.z * v.y), (t.z * v.x) - (t.x * v.z), (t.x * v.y) - (t.y * v.x)}; }
MF_VS_HD float norm_square(V3 v) { return v.x * v.x + v.y * v.y + v.z * v.z; }   // vectorbase.h:392-395
// norm, vectorbase.h:384-389: |v|^2 in float, the "== 1" test in double, the double sqrt rounded to float (which is sqrtf)
MF_VS_HD float norm3(V3 v) {
	const float l = v.x * v.x + v.y * v.y + v.z * v.z;
	const float eps2 = 1e-6f * 1e-6f;
	if (l <= eps2) return 0.f;
	return (fabs((double)l - 1.) < (double)eps2) ? 1.f : sqrtf(l);
}
// getNormalized, vectorbase.h:404-416: fac = (float)(1. / sqrt((double)l)), the epsilon branch returns the zero vector
MF_VS_HD V3 normalized(V3 v) {
	const float l = v.x * v.x + v.y * v.y + v.z * v.z;
	const float eps2 = 1e-6f * 1e-6f;
	if (fabs((double)l - 1.) < (double)eps2) return v;
	if (l > eps2) {
		const float fac = (float)(1. / sqrt((double)l));
		return {v.x * fac, v.y * fac, v.z * fac};
	}
	return {0.f, 0.f, 0.f};
}

// the mesh: triangles c[3][tcap] of node numbers, node positions pos[3][ncap] and flags[ncap]
struct MeshView {
	int64_t nTris, tcap, nNodes, ncap;
	const int32_t* tri;
	const float* pos;
	const int32_t* nflags;
};
// 0: triangle t names three nodes of the mesh
MF_VS_HD int tri_outside(const MeshView& M, int64_t t) {
	for (int c = 0; c < 3; c++) {
		const int32_t v = M.tri[c * M.tcap + t];
		if (v < 0 || v >= M.nNodes) return 1;
	}
	return 0;
}
MF_VS_HD V3 node_pos(const MeshView& M, int64_t v) { return {M.pos[v], M.pos[M.ncap + v], M.pos[2 * M.ncap + v]}; }
// getNode(tri, c), mesh.h:209
MF_VS_HD V3 tri_node(const MeshView& M, int64_t t, int c) { return node_pos(M, M.tri[c * M.tcap + t]); }
// getEdge, mesh.h:211
MF_VS_HD V3 tri_edge(const MeshView& M, int64_t t, int e) { return tri_node(M, t, (e + 1) % 3) - tri_node(M, t, e); }
// getFaceArea, mesh.h:213: 0.5 * norm(...) is a double product of a float, rounded back (exact)
MF_VS_HD float face_area(const MeshView& M, int64_t t) {
	const V3 c0 = tri_node(M, t, 0);
	return (float)(0.5 * (double)norm3(cross(tri_node(M, t, 1) - c0, tri_node(M, t, 2) - c0)));
}
// getFaceNormal, mesh.h:214
MF_VS_HD V3 face_normal(const MeshView& M, int64_t t) {
	const V3 c0 = tri_node(M, t, 0);
	return normalized(cross(tri_node(M, t, 1) - c0, tri_node(M, t, 2) - c0));
}
// getFaceCenter, mesh.h:215: the fp32 sum left to right, then `/ 3.0` -- each component divided in double and rounded once
MF_VS_HD V3 face_center(const MeshView& M, int64_t t) {
	const V3 s = (tri_node(M, t, 0) + tri_node(M, t, 1)) + tri_node(M, t, 2);
	return {(float)((double)s.x / 3.0), (float)((double)s.y / 3.0), (float)((double)s.z / 3.0)};
}
// isTriangleFixed, mesh.h:207 (NfFixed = 1)
MF_VS_HD int tri_fixed(const MeshView& M, int64_t t) {
	return ((M.nflags[M.tri[t]] & 1) || (M.nflags[M.tri[M.tcap + t]] & 1) || (M.nflags[M.tri[2 * M.tcap + t]] & 1)) ? 1 : 0;
}

MF_VS_HD V3 load3(const float* a, int64_t stride, int64_t i) { return {a[i], a[stride + i], a[2 * stride + i]}; }
MF_VS_HD void store3(float* a, int64_t stride, int64_t i, V3 v) {
	a[i] = v.x;
	a[stride + i] = v.y;
	a[2 * stride + i] = v.z;
}

// VortexSheetMesh::calcVorticity, vortexsheet.cpp:45-59, one triangle: `area < 1e-10` compares in double; smokeAmount = 0 in both
// branches; (c0 * e0 + c1 * e1 + c2 * e2) / area in fp32, left to right
MF_VS_HD V3 calc_vorticity(const MeshView& M, int64_t t, V3 circ) {
	const V3 e0 = tri_edge(M, t, 0), e1 = tri_edge(M, t, 1), e2 = tri_edge(M, t, 2);
	const float area = face_area(M, t);
	if ((double)area < 1e-10) return {0.f, 0.f, 0.f};
	return ((circ.x * e0 + circ.y * e1) + circ.z * e2) / area;
}

// vorticitySource, vortexplugins.cpp:95-117, one triangle; `a` is the acceleration sampled at the face centre (zero without vel: the
// reference then forms cross(fn, -gravity)).  Returns v, the norm taken after the update and before the clamp (what the statistics see).
MF_VS_HD float vorticity_source(const MeshView& M, int64_t t, int hasVel, V3 a, V3 gravity, float scale, float maxAmount, float mult,
                                float dt, float dx, V3& vort) {
	const V3 fn = face_normal(M, t);
	const V3 arg = hasVel ? (a - gravity) : V3{-gravity.x, -gravity.y, -gravity.z};
	V3 source = (-1.0f * cross(fn, arg)) * scale;
	if (tri_fixed(M, t)) source = {0.f, 0.f, 0.f};
	vort = vort * mult;
	vort = vort + (dt * source) / dx;
	const float v = norm3(vort);
	if (maxAmount > 0.f && v > maxAmount) vort = vort * (maxAmount / v);
	return v;
}

// smoothVorticity, vortexplugins.cpp:134-147, corner c of triangle i: the neighbour across the edge opposite to the corner and
// exp(|centre_t - centre_i|^2 * mult); weight 0 and index 0 where there is none.  The reference's exp is the float overload; this is
// the fp64 exp of the widened argument rounded once (DESIGN.md section 28 has the bound).
MF_VS_HD void smooth_weight(const MeshView& M, const int32_t* opposite, int64_t i, int c, float mult, float& w, int32_t& index) {
	const int32_t oc = opposite[3 * i + c];
	if (oc < 0) {
		w = 0.f;
		index = 0;
		return;
	}
	const int64_t t = oc / 3;
	const float arg = norm_square(face_center(M, t) - face_center(M, i)) * mult;
	w = (float)exp((double)arg);
	index = (int32_t)t;
}
// one triangle of one Jacobi pass, vortexplugins.cpp:153-163.  The weight of corner idx is read at weights[index[idx]] -- the array of
// 3 * nTris weights indexed by the neighbour TRIANGLE's number, as the reference writes it -- and not at weights[idx].
MF_VS_HD V3 smooth_pass(int64_t nTris, const float* weights, const int32_t* index, const float* vin, int64_t i) {
	float sum = 1.0f;
	V3 v = load3(vin, nTris, i);
	for (int c = 0; c < 3; c++) {
		const int64_t t = index[3 * i + c];
		const float w = weights[t];
		v = v + w * load3(vin, nTris, t);
		sum += w;
	}
	return v / sum;
}


// ---- VICintegration, vortexplugins.cpp:203-248: the Peskin spreading ----
struct Spread {
	int sx, sy, sz, sgi;
	float sigma, pkfac;      // pkfac = (Real)(M_PI / sigma)
	const int32_t* flags;
};
// One axis of the stencil: offset i of a centre coordinate p.  The skip tests are the reference's -- `p + i < 0` on the float sum,
// `(int)p + i >= size` on the truncated centre -- and the cell is the truncation of the float sum.  A float sum that rounds up onto
// `size` passes both tests in the reference, which then addresses a cell outside the grid: the precondition of the plugin excludes such
// centres, and the guard here leaves the cell out.
MF_VS_HD int spread_axis(float p, int i, int size, int& cell) {
	const float f = p + (float)i;
	if (f < 0.f || (int)p + i >= size) return 0;
	cell = (int)f;
	return cell < size;
}
// the weight term of one stencil cell before normalisation: 1.0 + cos(dl * pkfac) in double, or a negative value where dl > sigma.
// The reference's cos is the float overload; this is the fp64 cos of the widened fp32 product, rounded once to fp32.
MF_VS_HD double spread_term(const Spread& S, V3 pos, int i, int j, int k) {
	const V3 c = {(float)((double)i + 0.5 + (double)floorf(pos.x)), (float)((double)j + 0.5 + (double)floorf(pos.y)),
	              (float)((double)k + 0.5 + (double)floorf(pos.z))};
	const float dl = norm3(pos - c);
	if (dl > S.sigma) return -1.;
	const float arg = dl * S.pkfac;
	return 1.0 + (double)(float)cos((double)arg);
}
// pass A, one triangle: wnorm = 1.0 / sum over its own stencil in i, j, k order (infinite where nothing is fluid)
MF_VS_HD float spread_wnorm(const Spread& S, V3 pos) {
	float sum = 0.f;
	for (int i = -S.sgi; i < S.sgi; i++) {
		int cx, cy, cz;
		if (!spread_axis(pos.x, i, S.sx, cx)) continue;
		for (int j = -S.sgi; j < S.sgi; j++) {
			if (!spread_axis(pos.y, j, S.sy, cy)) continue;
			for (int k = -S.sgi; k < S.sgi; k++) {
				if (!spread_axis(pos.z, k, S.sz, cz)) continue;
				if (!(S.flags[((int64_t)cz * S.sy + cy) * S.sx + cx] & 1)) continue;
				const double term = spread_term(S, pos, i, j, k);
				if (term < 0.) continue;
				sum = (float)((double)sum + term);
			}
		}
	}
	return (float)(1.0 / (double)sum);
}
// pass B, what triangle (pos, v, wnorm) adds to the fluid cell (cx, cy, cz): acc += v * w for every stencil offset that lands there
MF_VS_HD void spread_add(const Spread& S, V3 pos, V3 v, float wnorm, int cx, int cy, int cz, V3& acc) {
	for (int i = -S.sgi; i < S.sgi; i++) {
		int x, y, z;
		if (!spread_axis(pos.x, i, S.sx, x) || x != cx) continue;
		for (int j = -S.sgi; j < S.sgi; j++) {
			if (!spread_axis(pos.y, j, S.sy, y) || y != cy) continue;
			for (int k = -S.sgi; k < S.sgi; k++) {
				if (!spread_axis(pos.z, k, S.sz, z) || z != cz) continue;
				const double term = spread_term(S, pos, i, j, k);
				if (term < 0.) continue;
				const float w = (float)(term * (double)wnorm);
				acc = acc + v * w;
			}
		}
	}
}
// the bin of a centre in the grid widened by m = sgi + 1 cells on every side; -1: the triangle reaches no cell (or is not a number)
MF_VS_HD int64_t spread_bin(const Spread& S, V3 pos) {
	const int m = S.sgi + 1;
	if (!(pos.x >= (float)-m && pos.x < (float)(S.sx + m) && pos.y >= (float)-m && pos.y < (float)(S.sy + m) && pos.z >= (float)-m && pos.z < (float)(S.sz + m)))
		return -1;
	const int bx = (int)floorf(pos.x) + m, by = (int)floorf(pos.y) + m, bz = (int)floorf(pos.z) + m;
	return ((int64_t)bz * (S.sy + 2 * m) + by) * (S.sx + 2 * m) + bx;
}

}  // namespace vsheet
}  // namespace mf
