// meshops_cells.h -- the per-corner, per-node and per-triangle bodies of meshops.hip as __host__ __device__ functions: the kernels call
// them with one thread per element, and a stand-alone host program (tools/meshops_host_check.hip) calls the same text in serial loops,
// where the host sanitizers can watch every index.  Contract and fp32 / fp64 map: DESIGN.md section 26.  Built with -ffp-contract=off.
#pragma once
#include "common.h"
#include <math.h>

namespace mf {
namespace meshops {

#define MF_HD __host__ __device__ __forceinline__

// the triangle list c[3][tcap] of a mesh with nNodes nodes
struct Tris {
	int64_t nTris, tcap, nNodes;
	const int32_t* tri;
};

// corner 3t + k: node = tri[t].c[k], next = 3t + (k + 1) % 3, prev = 3t + (k + 2) % 3 (mesh.cpp:243-251)
MF_HD int32_t corner_node(const Tris& T, int64_t c) { return T.tri[(c % 3) * T.tcap + c / 3]; }
MF_HD int32_t next_node(const Tris& T, int64_t c) { return T.tri[((c + 1) % 3) * T.tcap + c / 3]; }
MF_HD int32_t prev_node(const Tris& T, int64_t c) { return T.tri[((c + 2) % 3) * T.tcap + c / 3]; }

// 0: a triangle of three different nodes of the mesh; 1: a node number outside [0, nNodes); 2: a repeated node
MF_HD int tri_fault(const Tris& T, int64_t t) {
	const int32_t a = T.tri[t], b = T.tri[T.tcap + t], c = T.tri[2 * T.tcap + t];
	if (a < 0 || b < 0 || c < 0 || a >= T.nNodes || b >= T.nNodes || c >= T.nNodes) return 1;
	return (a == b || b == c || a == c) ? 2 : 0;
}

// the key of a corner: the unordered pair of its next and prev nodes, the edge opposite to it
MF_HD void edge_key(const Tris& T, int64_t c, int32_t& lo, int32_t& hi) {
	const int32_t a = next_node(T, c), b = prev_node(T, c);
	lo = a < b ? a : b;
	hi = a < b ? b : a;
}
MF_HD bool same_edge(const Tris& T, int64_t c, int64_t c2) {
	int32_t l, h, l2, h2;
	edge_key(T, c, l, h);
	edge_key(T, c2, l2, h2);
	return l == l2 && h == h2;
}

// Position s of the n corners sorted by key, ascending corner number within a key: a group c_1 < ... < c_g gets
// opposite[c_i] = c_{i+1} for i < g and opposite[c_g] = c_{g-1}, which is what the forward search of mesh.cpp:256-271 leaves; a group
// of one gets -1.  Returns bit 0 for a group of one and bit 1 at the head of a group of three or more.
MF_HD int group_entry(const Tris& T, int64_t n, const int32_t* sorted, int64_t s, int32_t* opposite) {
	const int32_t c = sorted[s];
	const bool head = s == 0 || !same_edge(T, sorted[s - 1], c);
	const bool tail = s == n - 1 || !same_edge(T, sorted[s + 1], c);
	opposite[c] = !tail ? sorted[s + 1] : (!head ? sorted[s - 1] : -1);
	int r = (head && tail) ? 1 : 0;
	if (head && s + 2 < n && same_edge(T, sorted[s + 2], c)) r |= 2;
	return r;
}

// 1-ring pairs: pair p = 2 * corner + which names (node of the corner, its next (which 0) or prev (which 1) node), mesh.cpp:286-290
MF_HD int32_t pair_node(const Tris& T, int64_t p) { return corner_node(T, p >> 1); }
MF_HD int32_t pair_neighbour(const Tris& T, int64_t p) { return (p & 1) ? prev_node(T, p >> 1) : next_node(T, p >> 1); }
// the first of its (node, neighbour) among the pairs sorted by node, then neighbour: the std::set keeps one
MF_HD int32_t pair_is_first(const Tris& T, const int32_t* sorted, int64_t s) {
	if (s == 0) return 1;
	const int32_t p = sorted[s], q = sorted[s - 1];
	return (pair_node(T, p) != pair_node(T, q) || pair_neighbour(T, p) != pair_neighbour(T, q)) ? 1 : 0;
}

// CSR offsets from a list sorted by node: entry s of m, of node `node` (its predecessor's node `before`, -1 for s == 0), is the
// rank-th value.  The first entry of a node closes the offsets of the nodes (before, node], the last entry those of (node, nNodes].
MF_HD void csr_offsets(int32_t* off, int64_t nNodes, int64_t s, int64_t m, int32_t before, int32_t node, int32_t rank, int32_t total) {
	if (node != before)
		for (int64_t v = (int64_t)before + 1; v <= node; v++) off[v] = rank;
	if (s == m - 1)
		for (int64_t v = (int64_t)node + 1; v <= nNodes; v++) off[v] = total;
}

// the arrays of the nodes, pos[3][ncap]
struct Nodes {
	int64_t n, ncap;
	const float* pos;
	const int32_t* flags;
};

// norm(), vectorbase.h:384-389
MF_HD float norm_of(float x, float y, float z) {
	const float l = x * x + y * y + z * z;
	const float eps2 = 1e-6f * 1e-6f;
	if (l <= eps2) return 0.f;
	return (fabs((double)l - 1.) < (double)eps2) ? 1.f : sqrtf(l);
}

// One node of one Jacobi step of smoothMesh (meshplugins.cpp:55-81): a node that no triangle names keeps the default-constructed
// Vec3 of the reference's `temp`, the origin; the others walk their ring ascending.  `edge * (1.0 / len)` has a double factor: each
// product is formed in double and rounded once; everything else is fp32.
MF_HD void smooth_node(const Nodes& N, const int32_t* nodeOff, const int32_t* ringNodes, const int32_t* triOff, int64_t p, float str,
                       float minLength, float out[3]) {
	if (triOff[p + 1] == triOff[p]) {
		out[0] = out[1] = out[2] = 0.f;
		return;
	}
	const float x = N.pos[p], y = N.pos[N.ncap + p], z = N.pos[2 * N.ncap + p];
	float dx = 0.f, dy = 0.f, dz = 0.f, totalLen = 0.f;
	for (int32_t q = nodeOff[p]; q < nodeOff[p + 1]; q++) {
		const int64_t j = ringNodes[q];
		const float ex = N.pos[j] - x, ey = N.pos[N.ncap + j] - y, ez = N.pos[2 * N.ncap + j] - z;
		const float len = norm_of(ex, ey, ez);
		if (len > minLength) {
			const double f = 1.0 / (double)len;
			dx += (float)((double)ex * f);
			dy += (float)((double)ey * f);
			dz += (float)((double)ez * f);
			totalLen += len;
		} else {
			totalLen = 0.f;
			break;
		}
	}
	out[0] = x;
	out[1] = y;
	out[2] = z;
	if (totalLen != 0.f) {
		const float w = str / totalLen;
		out[0] += dx * w;
		out[1] += dy * w;
		out[2] += dz * w;
	}
}

// The four fp64 terms of one triangle of Mesh::computeCenterOfMass (mesh.cpp:129-135): cvol = dot(cross(p1, p2), p3) / 6 and the three
// components of (p1 + p2 + p3) * (cvol / 4).
MF_HD void volume_terms(const Tris& T, int64_t ncap, const float* pos, int64_t t, double out[4]) {
	double p[3][3];
	for (int k = 0; k < 3; k++) {
		const int64_t v = T.tri[k * T.tcap + t];
		for (int c = 0; c < 3; c++) p[k][c] = (double)pos[c * ncap + v];
	}
	const double cx = p[0][1] * p[1][2] - p[0][2] * p[1][1];
	const double cy = p[0][2] * p[1][0] - p[0][0] * p[1][2];
	const double cz = p[0][0] * p[1][1] - p[0][1] * p[1][0];
	const double cvol = (cx * p[2][0] + cy * p[2][1] + cz * p[2][2]) / 6.0;
	const double q = cvol / 4.0;
	out[0] = cvol;
	for (int c = 0; c < 3; c++) out[1 + c] = ((p[0][c] + p[1][c]) + p[2][c]) * q;
}

// pos = origCM + (pos - newCM) * beta on a node without NfFixed (meshplugins.cpp:101-103), fp32
MF_HD float rescale_component(float x, float origCM, float newCM, float beta) { return origCM + (x - newCM) * beta; }

// ---- killSmallComponents (meshplugins.cpp:563-619) ----

// removeTri (mesh.cpp:401-448) over the tainted triangles in descending order, stated without the order: with K tainted triangles and
// below[q] = the number of tainted triangles < q, the removal of tainted q takes the then-last triangle, position nTris - (K - below[q]);
// that position holds its own triangle when it is not tainted, and what its own removal put there when it is.  So the kept slot h
// (tainted, h < nTris - K) ends with the triangle at the end of the chain q <- nTris - (K - below[q]) from h through tainted positions.
// q grows along the chain, and the chains of different slots share no position.
MF_HD int64_t hole_source(const int32_t* taint, const int32_t* below, int64_t nTris, int32_t K, int64_t h) {
	int64_t q = nTris - (K - below[h]);
	while (taint[q]) q = nTris - (K - below[q]);
	return q;
}

// corner c of a tainted triangle is where its node appears first among the tainted corners: the node's place in deletedNodes is the
// number of such corners before c (meshplugins.cpp:598-608)
MF_HD int32_t is_first_tainted_corner(const Tris& T, const int32_t* taint, const int32_t* firstCorner, int64_t c) {
	return (taint[c / 3] && firstCorner[corner_node(T, c)] == (int32_t)c) ? 1 : 0;
}

// removeNodes (mesh.cpp:457-484): newsize = nNodes - D; spotFlag[d] = deletedNodes[d] < newsize (a place to move to, in list order),
// keptFlag[i] = node newsize + i is not deleted (a node to move, ascending); the r-th kept node moves to the r-th spot
MF_HD int32_t node_new_index(const int32_t* keptFlag, const int32_t* keptRank, const int32_t* spot, int64_t i) {
	return keptFlag[i] ? spot[keptRank[i]] : -1;
}

}  // namespace meshops
}  // namespace mf
