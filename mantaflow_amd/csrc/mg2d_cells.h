// mg2d_cells.h -- the per-vertex bodies of mg2d.hip (the 2-D multigrid hierarchy, include/open/manta_hip_mg2d.h) as
// __host__ __device__ functions: the kernels of mg_driver.h call them, and tools/mg2d_host_check.hip runs the same text on the
// host, every launch replaced by a serial loop, for the host sanitizers.  (set_rhs and ordered_sum are in mg_host.h.)  Reference: source/multigrid.cpp, GridMg with
// mIs3D == false (cited per function).
//
// Layout.  Level 0 keeps a private SoA copy of the 5-point stencil in 3 planes (A0, Ai, Aj; x fastest) because trivial rows
// are rescaled; levels > 0 keep the 5 stored entries of the symmetric 9-point stencil as 5 planes (plane s = entry 4 + s of
// the 9-point stencil: centre, (+1, 0), (-1, +1), (0, +1), (+1, +1)).  Vertex types are one byte per vertex.
//
// Every pass of a V-cycle is a function over "work items start, start + stride, ...": a grid-wide kernel gives every thread
// one item, the single-workgroup tail kernel strides by its block size, the host check walks them one after the other.
#pragma once
#include "common.h"
#include "mg_host.h"

namespace mf {
namespace mg2d {

struct Lv {
	int sx, sy, n;
	float* A;            // level 0: 3 planes of n; levels > 0: 5 planes of n
	float *x, *b, *r;
	unsigned char* t;
};
struct View {
	int nl;
	Lv l[MAXL];
};
// one precomputed coarsening path (V) <-restriction- (U) <-A_0- (W) <-interpolation- (N), multigrid.cpp:286-312 with mDim = 2
struct Path {
	signed char N[2], U[2], W[2];
	signed char sc, sf, inU;
	float rw, iw;
};

MG_HD int odd2(int x, int y) { return (x & 1) + (y & 1); }

// ---------------------------------------------------------------------------------------------------------
// set-up
// ---------------------------------------------------------------------------------------------------------
// knCopyA + knActivateVertices + analyzeStencil with is3D == false (A[3] = A[6] = 0), multigrid.cpp:321-384, at vertex v.
// The reference scales the diagonal of trivial rows in place while other threads analyse their stencils; they only read the
// off-diagonals of their neighbours, which nobody changes.
MG_HD void copy_activate(const Lv& L, int v, const float* A0, const float* Ai, const float* Aj, int* info) {
	const int X = v % L.sx, Y = v / L.sx;
	float a[7];
	a[0] = A0[v];
	a[1] = Ai[v];
	a[2] = Aj[v];
	a[3] = 0.f;
	a[4] = X != 0 ? Ai[v - 1] : 0.f;
	a[5] = Y != 0 ? Aj[v - L.sx] : 0.f;
	a[6] = 0.f;
	unsigned char ty = vtInactive;
	float diag = a[0];
	if (a[0] != 0.f) {
		ty = vtActive;
		float smax = 0.f, ssum = 0.f;
		for (int i = 0; i < 7; i++) {
			ssum += a[i];
			smax = fmaxf(smax, fabsf(a[i]));
		}
		if (fabsf(ssum / smax) > 1E-6f) info[1] = 1;
		if (a[0] == 1.f && a[1] == 0.f && a[2] == 0.f && a[4] == 0.f && a[5] == 0.f) {
			ty = vtActiveTrivial;
			diag = a[0] * 1E-6f;      // mTrivialEquationScale
			info[2] = 1;
		}
	}
	L.t[v] = ty;
	L.A[v] = diag;
	L.A[L.n + v] = a[1];
	L.A[2 * L.n + v] = a[2];
}

// knGenCoarseGridOperator for l == 1, multigrid.cpp:594-614: the sorted paths, one after the other, into the 5 entries of V
MG_HD void operator1(const Lv& F, const Lv& C, int idx, const Path* paths, int npaths) {
	if (C.t[idx] == vtInactive) return;
	const int VX = idx % C.sx, VY = idx / C.sx;
	float acc = 0.f;
	int cur = 0;         // the paths are sorted by sc: one accumulator at a time
	for (int i = 0; i < npaths; i++) {
		const Path p = paths[i];
		if (p.sc != cur) {
			C.A[cur * C.n + idx] = acc;
			for (int s = cur + 1; s < p.sc; s++) C.A[s * C.n + idx] = 0.f;
			cur = p.sc;
			acc = 0.f;
		}
		const int nx = VX + p.N[0], ny = VY + p.N[1];
		if (nx < 0 || ny < 0 || nx >= C.sx || ny >= C.sy) continue;
		if (C.t[nx + C.sx * ny] == vtInactive) continue;
		const int ux = VX * 2 + p.U[0], uy = VY * 2 + p.U[1];
		if (ux < 0 || uy < 0 || ux >= F.sx || uy >= F.sy) continue;
		const int u = ux + F.sx * uy;
		if (F.t[u] == vtInactive) continue;
		const int wx = VX * 2 + p.W[0], wy = VY * 2 + p.W[1];
		if (wx < 0 || wy < 0 || wx >= F.sx || wy >= F.sy) continue;
		const int w = wx + F.sx * wy;
		if (F.t[w] == vtInactive) continue;
		const float a = F.A[p.sf * F.n + (p.inU ? u : w)];
		acc += p.rw * a * p.iw;
	}
	C.A[cur * C.n + idx] = acc;
	for (int s = cur + 1; s < 5; s++) C.A[s * C.n + idx] = 0.f;
}

// knGenCoarseGridOperator for l > 1, multigrid.cpp:615-656 (the reference's loop nest and its truncating divisions) over the
// 9-point neighbourhood: mStencilSize = 5, so the entries sc < 4 are left to the neighbours and entry sc is stored at sc - 4
MG_HD void operatorN(const Lv& F, const Lv& C, int idx) {
	if (C.t[idx] == vtInactive) return;
	const int VX = idx % C.sx, VY = idx / C.sx;
	for (int s = 0; s < 5; s++) C.A[s * C.n + idx] = 0.f;
	const int u0x = imax(0, VX * 2 - 1), u0y = imax(0, VY * 2 - 1);
	const int u1x = imin(F.sx - 1, VX * 2 + 1), u1y = imin(F.sy - 1, VY * 2 + 1);
	for (int uy = u0y; uy <= u1y; uy++)
	for (int ux = u0x; ux <= u1x; ux++) {
		const int u = ux + F.sx * uy;
		if (F.t[u] == vtInactive) continue;
		const float rw = pow2inv(odd2(ux, uy));
		const int n1x = imin(C.sx - 1, (ux + 2) / 2), n1y = imin(C.sy - 1, (uy + 2) / 2);
		for (int ny = (uy - 1) / 2; ny <= n1y; ny++)
		for (int nx = (ux - 1) / 2; nx <= n1x; nx++) {
			if (C.t[nx + C.sx * ny] == vtInactive) continue;
			const int sc = (nx - VX + 1) + 3 * (ny - VY + 1);
			if (sc < 4) continue;
			float* dstp = &C.A[(sc - 4) * C.n + idx];
			float acc = *dstp;
			const int w0x = imax(0, imax(ux - 1, nx * 2 - 1)), w0y = imax(0, imax(uy - 1, ny * 2 - 1));
			const int w1x = imin(F.sx - 1, imin(ux + 1, nx * 2 + 1)), w1y = imin(F.sy - 1, imin(uy + 1, ny * 2 + 1));
			for (int wy = w0y; wy <= w1y; wy++)
			for (int wx = w0x; wx <= w1x; wx++) {
				const int w = wx + F.sx * wy;
				if (F.t[w] == vtInactive) continue;
				const int sf = (wx - ux + 1) + 3 * (wy - uy + 1);
				const float iw = pow2inv(odd2(wx, wy));
				const float a = (sf < 5) ? F.A[(4 - sf) * F.n + w] : F.A[(sf - 4) * F.n + u];
				acc += rw * a * iw;
			}
			*dstp = acc;
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// the passes of a V-cycle over the work items start, start + stride, ...
// ---------------------------------------------------------------------------------------------------------
// b - (off-diagonal part of A x) at vertex v of level 0 in knSmoothColor's / knCalcResidual's order (d = 0, 1; the lower
// neighbour before the upper one), multigrid.cpp:684-689, 748-753
MG_HD float offdiag0(const Lv& L, int v, int X, int Y, float sum) {
	const float *Ai = L.A + L.n, *Aj = L.A + 2 * L.n;
	if (X > 0) sum -= Ai[v - 1] * L.x[v - 1];
	if (X < L.sx - 1) sum -= Ai[v] * L.x[v + 1];
	if (Y > 0) sum -= Aj[v - L.sx] * L.x[v - L.sx];
	if (Y < L.sy - 1) sum -= Aj[v] * L.x[v + L.sx];
	return sum;
}
// the 9-point row of a level > 0 at vertex v in the reference's s order (y, x from -1), multigrid.cpp:693-706, 756-767: the
// lower entries (s < 5) are read from the neighbour's row, the upper ones from the vertex's own.  SKIP_CENTRE: the smoother
// leaves s == 4 out.
template <bool SKIP_CENTRE>
MG_HD float row9_sub(const Lv& L, int v, int X, int Y, float sum) {
	int s = 0;
	for (int dy = -1; dy <= 1; dy++)
	for (int dx = -1; dx <= 1; dx++, s++) {
		if (SKIP_CENTRE && s == 4) continue;
		const int nx = X + dx, ny = Y + dy;
		if (nx < 0 || ny < 0 || nx >= L.sx || ny >= L.sy) continue;
		const int n = nx + L.sx * ny;
		if (L.t[n] == vtInactive) continue;
		const float a = (s < 5) ? L.A[(4 - s) * L.n + n] : L.A[(s - 4) * L.n + v];
		sum -= a * L.x[n];
	}
	return sum;
}

MG_HD int smooth_items(const Lv& L, bool l0) { return l0 ? ((L.sx + 1) >> 1) * L.sy : ((L.sx + 1) >> 1) * ((L.sy + 1) >> 1); }
MG_HD int smooth_colours(bool l0) { return l0 ? 2 : 4; }

// knSmoothColor, multigrid.cpp:668-711, one colour (smoothGS, :723-726).  Level 0: colour 0 is {(0,0), (1,1)} and colour 1
// {(1,0), (0,1)} of each 2 x 2 block, that is the parity (x + y) & 1 == colour; an item is a pair of x-neighbours, of which one
// has the colour.  Levels > 0: colour c is the single offset (c & 1, c >> 1) in the 2 x 2 blocks; an item is a block.
// Vertices of one colour do not read each other.
MG_HD void pass_smooth(const Lv& L, bool l0, int colour, int start, int stride) {
	const int items = smooth_items(L, l0);
	const int hx = (L.sx + 1) >> 1;
	for (int it = start; it < items; it += stride) {
		int X, Y;
		if (l0) {
			Y = it / hx;
			X = 2 * (it % hx) + ((Y + colour) & 1);
		} else {
			X = 2 * (it % hx) + (colour & 1);
			Y = 2 * (it / hx) + (colour >> 1);
		}
		if (X >= L.sx || Y >= L.sy) continue;
		const int v = X + L.sx * Y;
		if (L.t[v] == vtInactive) continue;
		const float sum = l0 ? offdiag0(L, v, X, Y, L.b[v]) : row9_sub<true>(L, v, X, Y, L.b[v]);
		L.x[v] = sum / L.A[v];
	}
}
// knCalcResidual, multigrid.cpp:739-771
MG_HD void pass_residual(const Lv& L, bool l0, int start, int stride) {
	for (int v = start; v < L.n; v += stride) {
		if (L.t[v] == vtInactive) continue;
		const int X = v % L.sx, Y = v / L.sx;
		float sum;
		if (l0) {
			sum = offdiag0(L, v, X, Y, L.b[v]);
			sum -= L.A[v] * L.x[v];
		} else {
			sum = row9_sub<false>(L, v, X, Y, L.b[v]);
		}
		L.r[v] = sum;
	}
}
// knRestrict (b of the coarse level from r of the fine one), multigrid.cpp:904-927, and knSet(x_coarse, 0), :472
MG_HD void pass_restrict(const Lv& F, const Lv& C, int start, int stride) {
	for (int idx = start; idx < C.n; idx += stride) {
		C.x[idx] = 0.f;
		if (C.t[idx] == vtInactive) continue;
		const int VX = idx % C.sx, VY = idx / C.sx;
		const int r0x = imax(0, VX * 2 - 1), r0y = imax(0, VY * 2 - 1);
		const int r1x = imin(F.sx - 1, VX * 2 + 1), r1y = imin(F.sy - 1, VY * 2 + 1);
		float sum = 0.f;
		for (int ry = r0y; ry <= r1y; ry++)
		for (int rx = r0x; rx <= r1x; rx++) {
			const int r = rx + F.sx * ry;
			if (F.t[r] == vtInactive) continue;
			sum += pow2inv(odd2(rx, ry)) * F.r[r];
		}
		C.b[idx] = sum;
	}
}
// knInterpolate into r of the fine level + knAddAssign(x, r), multigrid.cpp:484-486, 934-954.  The interpolated value is not
// stored: nothing reads r before the next residual pass overwrites it, and the inactive vertices (whose r stays 0) add 0.
MG_HD void pass_interp_add(const Lv& F, const Lv& C, int start, int stride) {
	for (int v = start; v < F.n; v += stride) {
		if (F.t[v] == vtInactive) continue;
		const int X = v % F.sx, Y = v / F.sx;
		float sum = 0.f;
		for (int iy = Y / 2; iy <= (Y + 1) / 2; iy++)
		for (int ix = X / 2; ix <= (X + 1) / 2; ix++) {
			const int i = ix + C.sx * iy;
			if (C.t[i] != vtInactive) sum += C.x[i];
		}
		const float c = pow2inv(odd2(X, Y)) * sum;
		F.x[v] = F.x[v] + c;
	}
}

// applyAStencil of solveCG (multigrid.cpp:798-826) on a double vector
MG_HD double cg_apply(const Lv& L, bool l0, int v, int X, int Y, const double* vec) {
	double sum = 0.0;
	if (l0) {
		const float *Ai = L.A + L.n, *Aj = L.A + 2 * L.n;
		if (X > 0) sum += Ai[v - 1] * vec[v - 1];
		if (X < L.sx - 1) sum += Ai[v] * vec[v + 1];
		if (Y > 0) sum += Aj[v - L.sx] * vec[v - L.sx];
		if (Y < L.sy - 1) sum += Aj[v] * vec[v + L.sx];
		sum += L.A[v] * vec[v];
	} else {
		int s = 0;
		for (int dy = -1; dy <= 1; dy++)
		for (int dx = -1; dx <= 1; dx++, s++) {
			const int nx = X + dx, ny = Y + dy;
			if (nx < 0 || ny < 0 || nx >= L.sx || ny >= L.sy) continue;
			const int n = nx + L.sx * ny;
			if (L.t[n] == vtInactive) continue;
			const float a = (s < 5) ? L.A[(4 - s) * L.n + n] : L.A[(s - 4) * L.n + v];
			sum += a * vec[n];
		}
	}
	return sum;
}

// ---------------------------------------------------------------------------------------------------------
// host helpers shared with the host check
// ---------------------------------------------------------------------------------------------------------
// the level pyramid of GridMg::GridMg with gridSize.z == 1, multigrid.cpp:256-276: sizes ((sx + 2) / 2, (sy + 2) / 2); no
// further level once both axes are <= 5 (z is 1) or the level has <= 1000 vertices.  Returns the number of levels.
inline int pyramid(int sx, int sy, int (*sizes)[2]) {
	int nl = 0;
	for (int l = 0; l < MAXL; l++) {
		if (l > 0) {
			const int px = sizes[l - 1][0], py = sizes[l - 1][1];
			if ((px <= 5 && py <= 5) || px * py <= 1000) break;
			sx = (px + 2) / 2;
			sy = (py + 2) / 2;
		}
		sizes[l][0] = sx;
		sizes[l][1] = sy;
		nl = l + 1;
	}
	return nl;
}

// The coarsening paths of level 1 in the reference's order, multigrid.cpp:286-318 with mDim = 2 and mStencilMin/Max.z = 0:
// V = (1, 1, 1), U over 3 x 3 at z = 2, the first five p7stencil entries, N in the plane z = 1, so s = N.x + 3 N.y + 9 and the
// kept paths (s >= 13) have sc = s - 13 in 0..4.  Generated U-major / stencil / N, then sorted by (sc, position of U) with
// std::sort -- the comparator leaves ties, and the operator sums in the resulting order, so the same generation order and the
// same algorithm are used here (the constant 9 * (U.z + 1) of the reference's key changes no comparison).
inline std::vector<Path> make_paths() {
	static const int p5[5][2] = {{0, 0}, {-1, 0}, {1, 0}, {0, -1}, {0, 1}};
	std::vector<Path> ps;
	for (int uy = 1; uy <= 3; uy++)
	for (int ux = 1; ux <= 3; ux++)
		for (int i = 0; i < 5; i++) {
			const int wx = ux + p5[i][0], wy = uy + p5[i][1];
			for (int ny = wy / 2; ny <= (wy + 1) / 2; ny++)
			for (int nx = wx / 2; nx <= (wx + 1) / 2; nx++) {
				const int s = nx + 3 * ny + 9;
				if (s < 13) continue;
				Path p;
				p.N[0] = nx - 1; p.N[1] = ny - 1;
				p.U[0] = ux - 2; p.U[1] = uy - 2;
				p.W[0] = wx - 2; p.W[1] = wy - 2;
				p.sc = s - 13;
				p.sf = (i + 1) / 2;
				p.inU = (i % 2 == 0);
				p.rw = 1.f / float(1 << ((ux % 2) + (uy % 2)));
				p.iw = 1.f / float(1 << ((wx % 2) + (wy % 2)));
				ps.push_back(p);
			}
		}
	auto less = [](const Path& a, const Path& b) {
		if (a.sc == b.sc) return (a.U[0] + 1) + 3 * (a.U[1] + 1) < (b.U[0] + 1) + 3 * (b.U[1] + 1);
		return a.sc < b.sc;
	};
	std::sort(ps.begin(), ps.end(), less);
	return ps;
}

inline MgDim dim_of(const Lv& L) { return MgDim{L.sx, L.sy, 1, L.n}; }

}  // namespace mg2d
}  // namespace mf
