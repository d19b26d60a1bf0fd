// meshsdf_cells.h -- the per-triangle, per-source and per-cell bodies of meshsdf.hip as __host__ __device__ functions: the kernels call
// them with one wave per triangle / one thread per source or cell, and a stand-alone host program (tools/meshsdf_host_check.hip) calls
// the same text in serial loops, where the host sanitizers can watch every index.  Contract and fp32 / fp64 map: DESIGN.md section 17.
// Built with -ffp-contract=off.  Reference: mesh.cpp:769-826, 868-1005.
#pragma once
#include "mesh_cells.h"

namespace mf {
namespace meshsdf {

using mesh::V3;

constexpr int OCC = 8;       // edge of an occupancy block, in cells
constexpr int TILE = 8;      // edge of a flood-fill tile
constexpr int HALO = TILE + 2;

struct TriView {
	int64_t nTris, tcap, nNodes, ncap;
	const int32_t* tri;
	const float* pos;
};

MF_HD V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }

// the three nodes of triangle t; false when one lies outside the node array
MF_HD bool tri_nodes(const TriView& T, int64_t t, V3 p[3]) {
	for (int c = 0; c < 3; c++) {
		const int64_t nd = T.tri[c * T.tcap + t];
		if (nd < 0 || nd >= T.nNodes) return false;
		p[c] = {T.pos[nd], T.pos[T.ncap + nd], T.pos[2 * T.ncap + nd]};
	}
	return true;
}

// norm, vectorbase.h:385-389, S = float: |v|^2 in fp32, 0 at or below eps^2, the "== 1" test in double
MF_HD float norm3(V3 v) {
	const float l = v.x * v.x + v.y * v.y + v.z * v.z;
	const float eps2 = 1e-6f * 1e-6f;
	if (l <= eps2) return 0.f;
	return fabs((double)l - 1.) < (double)eps2 ? 1.f : sqrtf(l);
}

// mesh.cpp:886-919: which corners the barycentric loops run over and how often; iterA == 0 where no edge is big.  wrap: a count that the
// reference's `short` does not hold
struct Plan {
	int big, iterA, iterB, pA, pB;
	bool wrap;
};
MF_HD Plan tri_plan(const V3 p[3]) {
	Plan P = {0, 0, 0, 0, 0, false};
	float len[3];
	for (int e = 0; e < 3; e++) {
		len[e] = norm3(sub(p[(e + 1) % 3], p[e]));     // getEdge(t, e) = node(e + 1) - node(e)
		if (len[e] > 0.75f) P.big += 1 << e;
	}
	if (P.big == 0) return P;
	const int n0 = (int)(len[1] * 0.75f), n1 = (int)(len[2] * 0.75f), n2 = (int)(len[0] * 0.75f);
	int a, b;
	if (!(P.big & 1)) {
		a = n1; P.pA = 0; b = n2; P.pB = 1;
	} else if (!(P.big & 2)) {
		a = n2; P.pA = 1; b = n0; P.pB = 2;
	} else {
		a = n0; P.pA = 2; b = n1; P.pB = 0;
	}
	P.wrap = a > 32767 || b > 32767 || !(len[0] < 65536.f && len[1] < 65536.f && len[2] < 65536.f);
	P.iterA = P.wrap ? 0 : a;
	P.iterB = P.wrap ? 0 : b;
	return P;
}

// mesh.cpp:924-927: u and v are double quotients rounded once, w = (1 - u) - v in fp32
MF_HD float sample_w(int s0, int iterA, int s1, int iterB, float* u, float* v) {
	*u = (float)((double)s0 / (double)iterA);
	*v = (float)((double)s1 / (double)iterB);
	return 1.f - *u - *v;
}

// the samples of row s0 that the reference keeps: the count pass and the emit pass both walk the row with sample_w
MF_HD int row_count(const Plan& P, int s0) {
	int c = 0;
	for (int s1 = 0; s1 < P.iterB; s1++) {
		float u, v;
		if (sample_w(s0, P.iterA, s1, P.iterB, &u, &v) < 0.f) continue;
		c++;
	}
	return c;
}

struct SrcOut {
	int64_t total, scap;
	float *pos, *nrm;
	float mx, my, mz;
};
MF_HD void put_source(const SrcOut& S, int64_t o, V3 p, V3 n) {
	if (o < 0 || o >= S.total) return;
	S.pos[o] = p.x; S.pos[S.scap + o] = p.y; S.pos[2 * S.scap + o] = p.z;
	S.nrm[o] = n.x; S.nrm[S.scap + o] = n.y; S.nrm[2 * S.scap + o] = n.z;
}
// getFaceNormal, mesh.h:214
MF_HD V3 face_normal(const V3 p[3]) {
	const V3 t = sub(p[1], p[0]), v = sub(p[2], p[0]);
	return mesh::normalized({t.y * v.z - t.z * v.y, t.z * v.x - t.x * v.z, t.x * v.y - t.y * v.x});
}
// getFaceCenter(t) * mult, mesh.h:215: the fp32 sum over a double 3.0, rounded once
MF_HD V3 face_centre(const V3 p[3], const SrcOut& S) {
	const float x = (float)((double)((p[0].x + p[1].x) + p[2].x) / 3.0), y = (float)((double)((p[0].y + p[1].y) + p[2].y) / 3.0),
	            z = (float)((double)((p[0].z + p[1].z) + p[2].z) / 3.0);
	return {x * S.mx, y * S.my, z * S.mz};
}
// mesh.cpp:930-932, the samples of row s0 from entry o on; -> the entry after the last one
MF_HD int64_t emit_row(const Plan& P, const V3 p[3], V3 n, int s0, int64_t o, const SrcOut& S) {
	const V3 a = p[P.pA], b = p[P.pB], c = p[3 - P.pA - P.pB];
	for (int s1 = 0; s1 < P.iterB; s1++) {
		float u, v;
		const float w = sample_w(s0, P.iterA, s1, P.iterB, &u, &v);
		if (w < 0.f) continue;
		const V3 q = {((a.x * S.mx) * u + (b.x * S.mx) * v) + (c.x * S.mx) * w, ((a.y * S.my) * u + (b.y * S.my) * v) + (c.y * S.my) * w,
		              ((a.z * S.mz) * u + (b.z * S.mz) * v) + (c.z * S.mz) * w};
		put_source(S, o++, q, n);
	}
	return o;
}

// _cIndex, mesh.cpp:822-826: truncation toward zero, then the bounds test; -1 outside.  A coordinate that no int holds (the x86
// conversion gives INT_MIN) and a NaN are outside
MF_HD int64_t cell_index(const Dim& d, float x, float y, float z) {
	if (!(fabsf(x) < 2e9f && fabsf(y) < 2e9f && fabsf(z) < 2e9f)) return -1;
	const int i = (int)x, j = (int)y, k = (int)z;
	if (i < 0 || j < 0 || k < 0 || i >= d.sx || j >= d.sy || k >= d.sz) return -1;
	return (int64_t)i + d.Y * j + d.Z * k;
}
MF_HD int occ_dim(int s) { return (s + OCC - 1) / OCC; }
MF_HD int64_t occ_index(const Dim& d, int i, int j, int k) {
	return (int64_t)(i / OCC) + (int64_t)occ_dim(d.sx) * ((j / OCC) + (int64_t)occ_dim(d.sy) * (k / OCC));
}

// the host scalars of meshSDF, mesh.cpp:870, 978-982, with the reference's types (Real = float)
struct Params {
	float cutoff, safeRadius2, cutoff2, isigma2;
	int intRadius;
};
static inline Params make_params(float sigma, float cutoff) {
	Params P;
	if (cutoff < 0) cutoff = 2 * sigma;
	P.cutoff = cutoff;
	const float safeRadius = (float)((double)cutoff + sqrt(3.0) * 0.5);
	P.safeRadius2 = safeRadius * safeRadius;
	P.cutoff2 = cutoff * cutoff;
	P.isigma2 = (float)(1.0 / (double)(sigma * sigma));
	P.intRadius = (int)((double)cutoff + 0.5);
	return P;
}

struct Gather {
	const float *pos, *nrm;
	int64_t scap;
	const int32_t *len, *start, *occ;
	Params P;
};
// does the clamped block of cell (cx, cy, cz) meet an occupied 8x8x8 block?
MF_HD bool any_source_near(const Dim& d, const Gather& G, int cx, int cy, int cz) {
	const int R = G.P.intRadius;
	const int i0 = (cx - R > 0 ? cx - R : 0) / OCC, i1 = (cx + R < d.sx - 1 ? cx + R : d.sx - 1) / OCC;
	const int j0 = (cy - R > 0 ? cy - R : 0) / OCC, j1 = (cy + R < d.sy - 1 ? cy + R : d.sy - 1) / OCC;
	const int k0 = (cz - R > 0 ? cz - R : 0) / OCC, k1 = (cz + R < d.sz - 1 ? cz + R : d.sz - 1) / OCC;
	const int64_t ox = occ_dim(d.sx), oy = occ_dim(d.sy);
	for (int k = k0; k <= k1; k++)
		for (int j = j0; j <= j1; j++)
			for (int i = i0; i <= i1; i++)
				if (G.occ[i + ox * (j + oy * k)]) return true;
	return false;
}
// SDFKernel at one cell, mesh.cpp:775-816, with levelset.setConst(-cutoff) folded in
MF_HD float gather_cell(const Dim& d, const Gather& G, int cx, int cy, int cz) {
	const Params& P = G.P;
	if (!any_source_near(d, G, cx, cy, cz)) return -P.cutoff;
	const float px = (float)cx + 0.5f, py = (float)cy + 0.5f, pz = (float)cz + 0.5f;
	float sum = 0.f, dist = 0.f;
	const int R = P.intRadius;
	const int i0 = cx - R > 0 ? cx - R : 0, i1 = cx + R < d.sx - 1 ? cx + R : d.sx - 1;
	const int j0 = cy - R > 0 ? cy - R : 0, j1 = cy + R < d.sy - 1 ? cy + R : d.sy - 1;
	const int k0 = cz - R > 0 ? cz - R : 0, k1 = cz + R < d.sz - 1 ? cz + R : d.sz - 1;
	for (int i = i0; i <= i1; i++)
		for (int j = j0; j <= j1; j++)
			for (int k = k0; k <= k1; k++) {
				const float dx = (float)(cx - i), dy = (float)(cy - j), dz = (float)(cz - k);
				if (dx * dx + dy * dy + dz * dz > P.safeRadius2) continue;
				const int64_t block = (int64_t)i + d.Y * j + d.Z * k;
				const int slen = G.len[block];
				if (slen == 0) continue;
				const int64_t s0 = G.start[block];
				for (int64_t s = s0; s < s0 + slen; s++) {
					const float rx = px - G.pos[s], ry = py - G.pos[G.scap + s], rz = pz - G.pos[2 * G.scap + s];
					const float r2 = rx * rx + ry * ry + rz * rz;
					if (r2 < P.cutoff2) {
						const float w = (float)exp((double)(-r2 * P.isigma2));
						sum += w;
						dist += (G.nrm[s] * rx + G.nrm[G.scap + s] * ry + G.nrm[2 * G.scap + s] * rz) * w;
					}
				}
			}
	return sum > 0.f ? dist / sum : -P.cutoff;
}

// ---- flood fill: the state of a cell inside a tile of TILE^3 cells with a halo of one; slot (lx, ly, lz) in [0, HALO)^3 is cell
// origin + l - 1.  0: neither, 1: candidate (value < 0), 2: flooded or seed (value == cutoff; seeds were set to cutoff before)
MF_HD int flood_state(const Dim& d, const float* __restrict__ phi, float cutoff, int ox, int oy, int oz, int slot) {
	const int lx = slot % HALO, ly = (slot / HALO) % HALO, lz = slot / (HALO * HALO);
	const int i = ox + lx - 1, j = oy + ly - 1, k = oz + lz - 1;
	if (i < 0 || j < 0 || k < 0 || i >= d.sx || j >= d.sy || k >= d.sz) return 0;
	const float v = phi[(int64_t)i + d.Y * j + d.Z * k];
	return v == cutoff ? 2 : (v < 0.f ? 1 : 0);
}
// a candidate with a flooded 6-neighbour floods; slot is an inner slot of the tile
MF_HD bool flood_step(const int* st, int slot) {
	return st[slot] == 1 && (st[slot - 1] == 2 || st[slot + 1] == 2 || st[slot - HALO] == 2 || st[slot + HALO] == 2 ||
	                         st[slot - HALO * HALO] == 2 || st[slot + HALO * HALO] == 2);
}

}  // namespace meshsdf
}  // namespace mf
