// mesh_cells.h -- the per-cell and per-node bodies of mesh.hip as __host__ __device__ functions: the kernels call them with one thread
// per cell / node, and a stand-alone host program (tools/mesh_host_check.hip) calls the same text in serial loops, where the host
// sanitizers can watch every index.  Contract and fp32 / fp64 map: DESIGN.md section 16.  Built with -ffp-contract=off.
#pragma once
#include "common.h"
#include <math.h>

namespace mf {
namespace mesh {

#define MF_HD __host__ __device__ __forceinline__
#ifdef __HIP_DEVICE_COMPILE__
#define MF_MESH_TABLE __device__ const
#else
#define MF_MESH_TABLE static const
#endif

// The classic marching-cubes triangle table (Lorensen & Cline; Bourke, "Polygonising a scalar field"), one 64-bit word per cube index:
// nibble q is the local edge number of triangle corner q, three per triangle, 0xf ends the list (at most five triangles).
MF_MESH_TABLE uint64_t TRI_WORDS[256] = {
	0xffffffffffffffffull, 0xfffffffffffff380ull, 0xfffffffffffff910ull, 0xffffffffff189381ull,
	0xfffffffffffffa21ull, 0xffffffffffa21380ull, 0xffffffffff920a29ull, 0xfffffff89a8a2382ull,
	0xfffffffffffff2b3ull, 0xffffffffff0b82b0ull, 0xffffffffffb32091ull, 0xfffffffb89b912b1ull,
	0xffffffffff3ab1a3ull, 0xfffffffab8a801a0ull, 0xfffffff9ab9b3093ull, 0xffffffffffb8aa89ull,
	0xfffffffffffff874ull, 0xffffffffff437034ull, 0xffffffffff748910ull, 0xfffffff137174914ull,
	0xffffffffff748a21ull, 0xfffffffa21403743ull, 0xfffffff748209a29ull, 0xffff4973727929a2ull,
	0xffffffffff2b3748ull, 0xfffffff40242b74bull, 0xfffffffb32748109ull, 0xffff1292b9b49b74ull,
	0xfffffff487ab31a3ull, 0xffff4b7401b41ab1ull, 0xffff30bab9b09874ull, 0xfffffffab99b4b74ull,
	0xfffffffffffff459ull, 0xffffffffff380459ull, 0xffffffffff051450ull, 0xfffffff513538458ull,
	0xffffffffff459a21ull, 0xfffffff594a21803ull, 0xfffffff204245a25ull, 0xffff8434535235a2ull,
	0xffffffffffb32459ull, 0xfffffff594b802b0ull, 0xfffffffb32510450ull, 0xffff584b82852512ull,
	0xfffffff45931ab3aull, 0xffffab81a8180594ull, 0xffff30bab5b05045ull, 0xfffffffb8aa85845ull,
	0xffffffffff975879ull, 0xfffffff375359039ull, 0xfffffff751710870ull, 0xffffffffff753351ull,
	0xfffffff21a759879ull, 0xffff37503505921aull, 0xffff25a758528208ull, 0xfffffff7533525a2ull,
	0xfffffff2b3987597ull, 0xffffb72029279759ull, 0xffff751871810b32ull, 0xfffffff51771b12bull,
	0xffffb3a31a758859ull, 0xf0aba010b7905075ull, 0xf07570805a30b0abull, 0xffffffffff5b75abull,
	0xfffffffffffff56aull, 0xffffffffff6a5380ull, 0xffffffffff6a5109ull, 0xfffffff6a5891381ull,
	0xffffffffff162561ull, 0xfffffff803621561ull, 0xfffffff620609569ull, 0xffff823625285895ull,
	0xffffffffff56ab32ull, 0xfffffff56a02b80bull, 0xfffffff6a5b32910ull, 0xffffb892b92916a5ull,
	0xfffffff315356b36ull, 0xffff6b51505b0b80ull, 0xffff9505606306b3ull, 0xfffffff89bb96956ull,
	0xffffffffff8746a5ull, 0xfffffffa56374034ull, 0xfffffff7486a5091ull, 0xffff49737179156aull,
	0xfffffff874156216ull, 0xffff743403625521ull, 0xffff620560509748ull, 0xf962695923497937ull,
	0xfffffff56a4872b3ull, 0xffffb720242746a5ull, 0xffff6a5b32874910ull, 0xf6a54b7b492b9129ull,
	0xffff6b51535b3748ull, 0xfb404b7b016b5b15ull, 0xf74836b630560950ull, 0xffff9b7974b96956ull,
	0xffffffffffa4694aull, 0xfffffff380a946a4ull, 0xfffffff04606a10aull, 0xffffa16468618138ull,
	0xfffffff462421941ull, 0xffff462942921803ull, 0xffffffffff624420ull, 0xfffffff624428238ull,
	0xfffffff32b46a94aull, 0xffff6a4a94b82280ull, 0xffffa164606102b3ull, 0xf1b8b12184a16146ull,
	0xffff36b319639469ull, 0xf14641916b0181b8ull, 0xfffffff4600636b3ull, 0xffffffffff86b846ull,
	0xfffffffa98a876a7ull, 0xffffa76a907a0370ull, 0xffff0818717a176aull, 0xfffffff37117a76aull,
	0xffff768981861621ull, 0xf937390976192962ull, 0xfffffff206607087ull, 0xffffffffff276237ull,
	0xffff76898a86ab32ull, 0xf7a9a76790b72702ull, 0xfb32a767a1871081ull, 0xffff17616a71b12bull,
	0xf63136b619768698ull, 0xffffffffff76b190ull, 0xffff06b0b3607087ull, 0xfffffffffffff6b7ull,
	0xfffffffffffffb67ull, 0xffffffffff67b803ull, 0xffffffffff67b910ull, 0xfffffff67b138918ull,
	0xffffffffff7b621aull, 0xfffffff7b6803a21ull, 0xfffffff7b69a2092ull, 0xffff89a38a3a27b6ull,
	0xffffffffff726327ull, 0xfffffff026067807ull, 0xfffffff910732672ull, 0xffff678891681261ull,
	0xfffffff73171a67aull, 0xffff801781a7167aull, 0xffff7a69a0a70730ull, 0xfffffff9a88a7a67ull,
	0xffffffffff68b486ull, 0xfffffff640603b63ull, 0xfffffff109648b68ull, 0xffff63b139369649ull,
	0xfffffff1a28b6486ull, 0xffff640b60b03a21ull, 0xffff9a2920b648b4ull, 0xf36463b34923a39aull,
	0xfffffff264248328ull, 0xffffffffff264240ull, 0xffff834642432091ull, 0xfffffff642241491ull,
	0xffff1a6648168318ull, 0xfffffff40660a01aull, 0xf39a9303a6834364ull, 0xffffffffff4a649aull,
	0xffffffffffb67594ull, 0xfffffff67b594380ull, 0xfffffffb67045105ull, 0xffff51345343867bull,
	0xfffffffb6721a459ull, 0xffff594380a217b6ull, 0xffff204a24a45b67ull, 0xf67b25a523453843ull,
	0xfffffff945267327ull, 0xffff786260680459ull, 0xffff045051673263ull, 0xf851584812786826ull,
	0xffff73167161a459ull, 0xf459078701671a61ull, 0xfa737a6a305a4a04ull, 0xffffa84a458a7a67ull,
	0xfffffff98b9b6596ull, 0xffff590650360b63ull, 0xffffb65510b508b0ull, 0xfffffff1355363b6ull,
	0xffff65b8b9b59a21ull, 0xfa21965690b603b0ull, 0xf52025a50865b58bull, 0xffff35a3a25363b6ull,
	0xffff283265825985ull, 0xfffffff260069659ull, 0xf826283865081851ull, 0xffffffffff612651ull,
	0xf698965683a61631ull, 0xffff06505960a01aull, 0xffffffffffa65830ull, 0xfffffffffffff65aull,
	0xffffffffffb57a5bull, 0xfffffff03857ba5bull, 0xfffffff091ba57b5ull, 0xffff1381897ba57aull,
	0xfffffff15717b21bull, 0xffffb27571721380ull, 0xffff7b2209729579ull, 0xf289823295b27257ull,
	0xfffffff573532a52ull, 0xffff52a578258028ull, 0xffff2a37353a5109ull, 0xf25752a278129289ull,
	0xffffffffff573531ull, 0xfffffff571170780ull, 0xfffffff735539309ull, 0xffffffffff795789ull,
	0xfffffff8ba8a5485ull, 0xffff03bba50b5405ull, 0xffff54aba8a48910ull, 0xf41314943b54a4baull,
	0xffff8548b2582152ull, 0xfb151b2b543b0b40ull, 0xf58b8545b2950520ull, 0xffffffffff3b2549ull,
	0xffff483543253a52ull, 0xfffffff0244252a5ull, 0xf910854583a532a3ull, 0xffff2492914252a5ull,
	0xfffffff153358548ull, 0xffffffffff501540ull, 0xffff530509358548ull, 0xfffffffffffff549ull,
	0xfffffffba9b947b4ull, 0xffffba97b9794380ull, 0xffffb470414b1ba1ull, 0xf4bab474a1843413ull,
	0xffff219b294b97b4ull, 0xf3801b2b197b9479ull, 0xfffffff04224b47bull, 0xffff42343824b47bull,
	0xffff947732972a92ull, 0xf70207872a4797a9ull, 0xfa040a1a472a3a73ull, 0xffffffffff4782a1ull,
	0xfffffff317714194ull, 0xffff178180714194ull, 0xffffffffff347304ull, 0xfffffffffffff784ull,
	0xffffffffff8ba8a9ull, 0xfffffffa9bb93903ull, 0xfffffffba88a0a10ull, 0xffffffffffa3ba13ull,
	0xfffffff8b99b1b21ull, 0xffff9b2921b93903ull, 0xffffffffffb08b20ull, 0xfffffffffffffb23ull,
	0xfffffff98aa82832ull, 0xffffffffff2902a9ull, 0xffff8a1810a82832ull, 0xfffffffffffff2a1ull,
	0xffffffffff819831ull, 0xfffffffffffff190ull, 0xfffffffffffff830ull, 0xffffffffffffffffull,
};

// corner l of a cell sits at (cx, cy, cz)(l) from the cell; local edge e joins corners e1(e) -> e2(e)
MF_HD int cx(int l) { return ((l + 1) >> 1) & 1; }
MF_HD int cy(int l) { return (l >> 1) & 1; }
MF_HD int cz(int l) { return l >> 2; }
MF_HD int e1(int e) { return e < 8 ? e : e - 8; }
MF_HD int e2(int e) { return e < 4 ? ((e + 1) & 3) : (e < 8 ? 4 + ((e - 3) & 3) : e - 4); }
MF_HD int edge_axis(int e) { return e < 8 ? (e & 1) : 2; }

MF_HD int tri_count(unsigned c) {
	const uint64_t w = TRI_WORDS[c];
	int t = 0;
	while (t < 5 && ((w >> (12 * t)) & 15) != 15) t++;
	return t;
}

// the cube index of cell (i, j, k), 0 for an inactive cell (levelset.cpp:346-360)
MF_HD unsigned classify_cell(const Dim& d, const float* __restrict__ phi, int i, int j, int k) {
	if (i >= d.sx - 1 || j >= d.sy - 1 || k >= d.sz - 1) return 0;
	unsigned c = 0;
	bool skip = false;
	for (int l = 0; l < 8; l++) {
		const float p = phi[(int64_t)(i + cx(l)) + d.Y * (j + cy(l)) + d.Z * (k + cz(l))];
		const float v = -p;
		if (p <= -1000.f) skip = true;
		if (v < 1e-4f) c |= 1u << l;
	}
	return (skip || c == 255u) ? 0u : c;
}

// The first active cell, in sweep order, of the cells that share local edge e of the active cell (i, j, k): -> its index, and *le = the
// edge's local number there.  With p < q the two axes across the edge and o the lower corner of the edge, the sharing cells are at
// (o_p - 1, o_q - 1), (o_p, o_q - 1), (o_p - 1, o_q), (o_p, o_q) from the cell, which is their sweep order; the cell itself is one of them.
// A neighbour at +1 lies inside the array (an active cell has i < sx-1 ...), a neighbour at -1 is checked.
MF_HD int64_t edge_owner(const Dim& d, const uint8_t* __restrict__ cube, int i, int j, int k, int e, int* le) {
	const int a = e1(e), b = e2(e), axis = edge_axis(e);
	const int o[3] = {cx(a) < cx(b) ? cx(a) : cx(b), cy(a) < cy(b) ? cy(a) : cy(b), cz(a) < cz(b) ? cz(a) : cz(b)};
	const int p = axis == 0 ? 1 : 0, q = axis == 2 ? 1 : 2;
	const int cell[3] = {i, j, k};
	for (int dq = 1; dq >= 0; dq--)
		for (int dp = 1; dp >= 0; dp--) {
			int off[3] = {0, 0, 0};
			off[p] = o[p] - dp;
			off[q] = o[q] - dq;
			const int ci = cell[0] + off[0], cj = cell[1] + off[1], ck = cell[2] + off[2];
			const bool self = off[p] == 0 && off[q] == 0;
			if (!self && (ci < 0 || cj < 0 || ck < 0)) continue;
			const int64_t cidx = (int64_t)ci + d.Y * cj + d.Z * ck;
			if (self || cube[cidx] != 0) {
				*le = axis == 0 ? 2 * dp + 4 * dq : (axis == 1 ? 3 - 2 * dp + 4 * dq : 8 + (dq ? 3 - dp : dp));
				return cidx;
			}
		}
	*le = e;    // not reached: the cell itself is in the list
	return (int64_t)i + d.Y * j + d.Z * k;
}

// the crossed edges of the active cell (i, j, k), cube index c, that no earlier active cell shares
MF_HD unsigned owned_mask(const Dim& d, const uint8_t* __restrict__ cube, int i, int j, int k, unsigned c) {
	unsigned m = 0;
	const int64_t idx = (int64_t)i + d.Y * j + d.Z * k;
	for (int e = 0; e < 12; e++) {
		if ((((c >> e1(e)) ^ (c >> e2(e))) & 1u) == 0) continue;
		int le;
		if (edge_owner(d, cube, i, j, k, e, &le) == idx) m |= 1u << e;
	}
	return m;
}

struct V3 {
	float x, y, z;
};
// getGradient, grid.h:556-572, 3-D: central differences without the 1/2; i and j are clamped to [1, size - 2] (upper clamp first), the
// x and y differences are taken in the plane k as given, and only the z difference clamps k
MF_HD V3 gradient(const Dim& d, const float* __restrict__ phi, int i, int j, int k) {
	if (i > d.sx - 2) i = d.sx - 2;
	if (j > d.sy - 2) j = d.sy - 2;
	if (i < 1) i = 1;
	if (j < 1) j = 1;
	const int64_t xy = (int64_t)i + d.Y * j + d.Z * k;
	if (k > d.sz - 2) k = d.sz - 2;
	if (k < 1) k = 1;
	const int64_t idx = (int64_t)i + d.Y * j + d.Z * k;
	return {phi[xy + 1] - phi[xy - 1], phi[xy + d.Y] - phi[xy - d.Y], phi[idx + d.Z] - phi[idx - d.Z]};
}
// getNormalized, vectorbase.h:405-416, S = float: |v|^2 in fp32, the "== 1" test in double, fac = (float)(1. / sqrt((double)l)): the
// header's template sees the double sqrt only
MF_HD V3 normalized(V3 v) {
	const float l = v.x * v.x + v.y * v.y + v.z * v.z;
	const float eps2 = 1e-6f * 1e-6f;
	if (fabs((double)l - 1.) < (double)eps2) return v;
	if (l > eps2) {
		const float fac = (float)(1. / sqrt((double)l));
		return {v.x * fac, v.y * fac, v.z * fac};
	}
	return {0.f, 0.f, 0.f};
}

// the node of local edge e of cell (i, j, k), levelset.cpp:376-389
MF_HD void edge_node(const Dim& d, const float* __restrict__ phi, int i, int j, int k, int e, V3* pos, V3* nrm) {
	const int a = e1(e), b = e2(e);
	const int ai = i + cx(a), aj = j + cy(a), ak = k + cz(a), bi = i + cx(b), bj = j + cy(b), bk = k + cz(b);
	const float va = -phi[(int64_t)ai + d.Y * aj + d.Z * ak], vb = -phi[(int64_t)bi + d.Y * bj + d.Z * bk];
	const float mu = (1e-4f - va) / (vb - va);
	pos->x = (float)ai + ((float)bi - (float)ai) * mu + 0.5f;
	pos->y = (float)aj + ((float)bj - (float)aj) * mu + 0.5f;
	pos->z = (float)ak + ((float)bk - (float)ak) * mu + 0.5f;
	const V3 g1 = gradient(d, phi, ai, aj, ak), g2 = gradient(d, phi, bi, bj, bk);
	const double w1 = 1.0 - (double)mu;     // `* (1.0 - mu)`: Vector3D<float> * double, each product rounded once
	const V3 n = {(float)((double)g1.x * w1) + g2.x * mu, (float)((double)g1.y * w1) + g2.y * mu, (float)((double)g1.z * w1) + g2.z * mu};
	*nrm = normalized(n);
}

struct MeshOut {
	int64_t nNodes, nTris, ncap, tcap;
	float *pos, *normal;
	int32_t *nflags, *tri, *tflags;
};
// the emit pass at an active cell: its owned nodes, then its triangles
MF_HD void emit_cell(const Dim& d, const float* __restrict__ phi, const uint8_t* __restrict__ cube, const uint16_t* __restrict__ mask,
                     const int32_t* __restrict__ nodeOff, const int32_t* __restrict__ triOff, int i, int j, int k, const MeshOut& M) {
	const int64_t idx = (int64_t)i + d.Y * j + d.Z * k;
	const unsigned c = cube[idx];
	if (c == 0) return;
	const unsigned m = mask[idx];
	int64_t nd = nodeOff[idx];
	for (int e = 0; e < 12; e++) {
		if (!((m >> e) & 1u)) continue;
		V3 p, n;
		edge_node(d, phi, i, j, k, e, &p, &n);
		if (nd < M.nNodes) {
			M.pos[nd] = p.x;
			M.pos[M.ncap + nd] = p.y;
			M.pos[2 * M.ncap + nd] = p.z;
			M.normal[nd] = n.x;
			M.normal[M.ncap + nd] = n.y;
			M.normal[2 * M.ncap + nd] = n.z;
			M.nflags[nd] = 0;
		}
		nd++;
	}
	const uint64_t w = TRI_WORDS[c];
	int64_t t = triOff[idx];
	for (int q = 0; q < 15 && ((w >> (4 * q)) & 15) != 15; q += 3, t++) {
		if (t >= M.nTris) continue;
		for (int r = 0; r < 3; r++) {
			int le;
			const int64_t o = edge_owner(d, cube, i, j, k, (int)((w >> (4 * (q + r))) & 15), &le);
			M.tri[r * M.tcap + t] = nodeOff[o] + __builtin_popcount((unsigned)mask[o] & ((1u << le) - 1u));
		}
		M.tflags[t] = 0;
	}
}

// ---- Mesh::advectInGrid ---------------------------------------------------------------------------------------------------------
// FlagGrid::isInBounds(pos, bnd), grid.h:65 + 84-91: toVec3i truncates
MF_HD bool in_bounds_pos(const Dim& d, float x, float y, float z, int bnd) {
	const int i = (int)x, j = (int)y, k = (int)z;
	bool r = i >= bnd && j >= bnd && i < d.sx - bnd && j < d.sy - bnd;
	if (d.is3d)
		r = r && (k >= bnd && k < d.sz - bnd);
	else
		r = r && (k == 0);
	return r;
}

// one axis pair of Mesh::rotate, mesh.cpp:359-363
MF_HD void rotate_pair(float* a, float* b, float sin_t, float cos_t) {
	const float fa = *a, fb = *b;
	*a = fa * cos_t - fb * sin_t;
	*b = fb * cos_t + fa * sin_t;
}

}  // namespace mesh
}  // namespace mf
