// mg3d_cells.h -- the per-vertex bodies of multigrid.hip (the 3-D multigrid hierarchy, include/manta_hip_multigrid.h) as
// __host__ __device__ functions under the names mg2d_cells.h uses for the 2-D ones: the kernels of mg_driver.h call them.
// Reference: source/multigrid.{h,cpp} (GridMg, cited per function).
//
// Layout.  Level 0 keeps a private SoA copy of the 7-point stencil (planes A0, Ai, Aj, Ak; x fastest) because trivial rows
// are rescaled; levels > 0 keep the 14 stored entries of the symmetric 27-point stencil as 14 planes, so the 64 vertices of a
// wavefront read 14 coalesced streams.  Vertex types are one byte per vertex.
//
// Every pass of a V-cycle is a function over the work items begin + start, begin + start + stride, ... below end: a grid-wide
// kernel gives every thread one item of [0, items), the single-workgroup tail kernel strides over them by its block size, and
// the ranged kernels of mgslab.hip give every thread one item of a sub-range.  The items of every pass are Z-major, so the
// planes [z0, z1) of a level are the items [z0 * (items per plane), z1 * (items per plane)).
#pragma once
#include "common.h"
#include "mg_host.h"

namespace mf {
namespace mg3d {

struct Lv {
	int sx, sy, sz, n;
	float* A;            // level 0: 4 planes of n; levels > 0: 14 planes of n
	float *x, *b, *r;
	unsigned char* t;
};
struct View {
	int nl;
	Lv l[MAXL];
};
// one precomputed coarsening path (V) <-restriction- (U) <-A_0- (W) <-interpolation- (N), multigrid.cpp:286-312
struct Path {
	signed char N[3], U[3], W[3];
	signed char sc, sf, inU;
	float rw, iw;
};

MG_HD int odd3(int x, int y, int z) { return (x & 1) + (y & 1) + (z & 1); }

// ---------------------------------------------------------------------------------------------------------
// set-up
// ---------------------------------------------------------------------------------------------------------
// knCopyA + knActivateVertices + analyzeStencil, multigrid.cpp:321-384, at vertex v.  The reference scales the diagonal of
// trivial rows in place while other threads analyse their stencils; they only read the off-diagonals of their neighbours,
// which nobody changes.
MG_HD void copy_activate(const Lv& L, int v, const float* A0, const float* Ai, const float* Aj, const float* Ak, int* info) {
	const int X = v % L.sx, Y = (v / L.sx) % L.sy, Z = v / (L.sx * L.sy);
	const int py = L.sx, pz = L.sx * L.sy;
	float a[7];
	a[0] = A0[v];
	a[1] = Ai[v];
	a[2] = Aj[v];
	a[3] = Ak[v];
	a[4] = X != 0 ? Ai[v - 1] : 0.f;
	a[5] = Y != 0 ? Aj[v - py] : 0.f;
	a[6] = Z != 0 ? Ak[v - pz] : 0.f;
	unsigned char ty = vtInactive;
	float diag = a[0];
	if (a[0] != 0.f) {
		ty = vtActive;
		float smax = 0.f, ssum = 0.f;
#pragma unroll
		for (int i = 0; i < 7; i++) {
			ssum += a[i];
			smax = fmaxf(smax, fabsf(a[i]));
		}
		if (fabsf(ssum / smax) > 1E-6f) info[1] = 1;
		if (a[0] == 1.f && a[1] == 0.f && a[2] == 0.f && a[3] == 0.f && a[4] == 0.f && a[5] == 0.f && a[6] == 0.f) {
			ty = vtActiveTrivial;
			diag = a[0] * 1E-6f;      // mTrivialEquationScale
			info[2] = 1;
		}
	}
	L.t[v] = ty;
	L.A[v] = diag;
	L.A[L.n + v] = a[1];
	L.A[2 * L.n + v] = a[2];
	L.A[3 * L.n + v] = a[3];
}

// knGenCoarseGridOperator for l == 1, multigrid.cpp:594-614: the sorted paths, one after the other, into the 14 entries of V.
// (The levels by value: with references the compiler splits the six bounds tests of N over two branches per path.)
MG_HD void operator1(const Lv F, const Lv C, int idx, const Path* paths, int npaths) {
	if (C.t[idx] == vtInactive) return;
	const int VX = idx % C.sx, VY = (idx / C.sx) % C.sy, VZ = idx / (C.sx * C.sy);
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
		const int nx = VX + p.N[0], ny = VY + p.N[1], nz = VZ + p.N[2];
		if (nx < 0 || ny < 0 || nz < 0 || nx >= C.sx || ny >= C.sy || nz >= C.sz) continue;
		if (C.t[nx + C.sx * (ny + C.sy * nz)] == vtInactive) continue;
		const int ux = VX * 2 + p.U[0], uy = VY * 2 + p.U[1], uz = VZ * 2 + p.U[2];
		if (ux < 0 || uy < 0 || uz < 0 || ux >= F.sx || uy >= F.sy || uz >= F.sz) continue;
		const int u = ux + F.sx * (uy + F.sy * uz);
		if (F.t[u] == vtInactive) continue;
		const int wx = VX * 2 + p.W[0], wy = VY * 2 + p.W[1], wz = VZ * 2 + p.W[2];
		if (wx < 0 || wy < 0 || wz < 0 || wx >= F.sx || wy >= F.sy || wz >= F.sz) continue;
		const int w = wx + F.sx * (wy + F.sy * wz);
		if (F.t[w] == vtInactive) continue;
		const float a = F.A[p.sf * F.n + (p.inU ? u : w)];
		acc += p.rw * a * p.iw;
	}
	C.A[cur * C.n + idx] = acc;
	for (int s = cur + 1; s < 14; s++) C.A[s * C.n + idx] = 0.f;
}

// knGenCoarseGridOperator for l > 1, multigrid.cpp:615-656 (the reference's loop nest and its truncating divisions)
MG_HD void operatorN(const Lv& F, const Lv& C, int idx) {
	if (C.t[idx] == vtInactive) return;
	const int VX = idx % C.sx, VY = (idx / C.sx) % C.sy, VZ = idx / (C.sx * C.sy);
	for (int s = 0; s < 14; s++) C.A[s * C.n + idx] = 0.f;
	const int u0x = imax(0, VX * 2 - 1), u0y = imax(0, VY * 2 - 1), u0z = imax(0, VZ * 2 - 1);
	const int u1x = imin(F.sx - 1, VX * 2 + 1), u1y = imin(F.sy - 1, VY * 2 + 1), u1z = imin(F.sz - 1, VZ * 2 + 1);
	for (int uz = u0z; uz <= u1z; uz++)
	for (int uy = u0y; uy <= u1y; uy++)
	for (int ux = u0x; ux <= u1x; ux++) {
		const int u = ux + F.sx * (uy + F.sy * uz);
		if (F.t[u] == vtInactive) continue;
		const float rw = pow2inv(odd3(ux, uy, uz));
		const int n1x = imin(C.sx - 1, (ux + 2) / 2), n1y = imin(C.sy - 1, (uy + 2) / 2), n1z = imin(C.sz - 1, (uz + 2) / 2);
		for (int nz = (uz - 1) / 2; nz <= n1z; nz++)
		for (int ny = (uy - 1) / 2; ny <= n1y; ny++)
		for (int nx = (ux - 1) / 2; nx <= n1x; nx++) {
			const int nn = nx + C.sx * (ny + C.sy * nz);
			if (C.t[nn] == vtInactive) continue;
			const int sc = (nx - VX + 1) + 3 * (ny - VY + 1) + 9 * (nz - VZ + 1);
			if (sc < 13) continue;
			float* dstp = &C.A[(sc - 13) * C.n + idx];
			float acc = *dstp;
			const int w0x = imax(0, imax(ux - 1, nx * 2 - 1)), w0y = imax(0, imax(uy - 1, ny * 2 - 1)), w0z = imax(0, imax(uz - 1, nz * 2 - 1));
			const int w1x = imin(F.sx - 1, imin(ux + 1, nx * 2 + 1)), w1y = imin(F.sy - 1, imin(uy + 1, ny * 2 + 1)),
			          w1z = imin(F.sz - 1, imin(uz + 1, nz * 2 + 1));
			for (int wz = w0z; wz <= w1z; wz++)
			for (int wy = w0y; wy <= w1y; wy++)
			for (int wx = w0x; wx <= w1x; wx++) {
				const int w = wx + F.sx * (wy + F.sy * wz);
				if (F.t[w] == vtInactive) continue;
				const int sf = (wx - ux + 1) + 3 * (wy - uy + 1) + 9 * (wz - uz + 1);
				const float iw = pow2inv(odd3(wx, wy, wz));
				const float a = (sf < 14) ? F.A[(13 - sf) * F.n + w] : F.A[(sf - 13) * F.n + u];
				acc += rw * a * iw;
			}
			*dstp = acc;
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// the passes of a V-cycle over the work items start, start + stride, ...
// ---------------------------------------------------------------------------------------------------------
// b - (off-diagonal part of A x) at vertex v of level 0 in knSmoothColor's / knCalcResidual's order, multigrid.cpp:684-689, 748-753
MG_HD float offdiag0(const Lv& L, int v, int X, int Y, int Z, float sum) {
	const int py = L.sx, pz = L.sx * L.sy;
	const float *Ai = L.A + L.n, *Aj = L.A + 2 * L.n, *Ak = L.A + 3 * L.n;
	if (X > 0) sum -= Ai[v - 1] * L.x[v - 1];
	if (X < L.sx - 1) sum -= Ai[v] * L.x[v + 1];
	if (Y > 0) sum -= Aj[v - py] * L.x[v - py];
	if (Y < L.sy - 1) sum -= Aj[v] * L.x[v + py];
	if (Z > 0) sum -= Ak[v - pz] * L.x[v - pz];
	if (Z < L.sz - 1) sum -= Ak[v] * L.x[v + pz];
	return sum;
}
// the 27-point row of a level > 0 at vertex v in the reference's s order (z, y, x from -1), multigrid.cpp:693-706, 756-767.
// SKIP_CENTRE: the smoother leaves s == 13 out.
template <bool SKIP_CENTRE>
MG_HD float row27_sub(const Lv& L, int v, int X, int Y, int Z, float sum) {
	int s = 0;
	for (int dz = -1; dz <= 1; dz++)
	for (int dy = -1; dy <= 1; dy++)
	for (int dx = -1; dx <= 1; dx++, s++) {
		if (SKIP_CENTRE && s == 13) continue;
		const int nx = X + dx, ny = Y + dy, nz = Z + dz;
		if (nx < 0 || ny < 0 || nz < 0 || nx >= L.sx || ny >= L.sy || nz >= L.sz) continue;
		const int n = nx + L.sx * (ny + L.sy * nz);
		if (L.t[n] == vtInactive) continue;
		const float a = (s < 14) ? L.A[(13 - s) * L.n + n] : L.A[(s - 13) * L.n + v];
		sum -= a * L.x[n];
	}
	return sum;
}

MG_HD int smooth_items(const Lv& L, bool l0) { return l0 ? ((L.sx + 1) / 2) * L.sy * L.sz : ((L.sx + 1) / 2) * ((L.sy + 1) / 2) * ((L.sz + 1) / 2); }
MG_HD int smooth_colours(bool l0) { return l0 ? 2 : 8; }

// knSmoothColor, multigrid.cpp:668-711, one colour.  Level 0: colour c is the parity (x + y + z) & 1 == c (the offsets
// {000, 110, 101, 011} and {100, 010, 001, 111}); an item is a pair of x-neighbours, of which one has the colour.  Levels > 0:
// colour c is the offset (c & 1, c >> 1 & 1, c >> 2) in the 2 x 2 x 2 blocks; an item is a block.  Vertices of one colour do
// not read each other.
MG_HD void pass_smooth(const Lv& L, bool l0, int colour, int begin, int end, int start, int stride) {
	if (l0) {
		const int hx = (L.sx + 1) >> 1;
		for (int it = begin + start; it < end; it += stride) {
			const int q = it % hx, Y = (it / hx) % L.sy, Z = it / (hx * L.sy);
			const int X = 2 * q + ((Y + Z + colour) & 1);
			if (X >= L.sx) continue;
			const int v = X + L.sx * (Y + L.sy * Z);
			if (L.t[v] == vtInactive) continue;
			const float sum = offdiag0(L, v, X, Y, Z, L.b[v]);
			L.x[v] = sum / L.A[v];
		}
	} else {
		const int bx = (L.sx + 1) >> 1, by = (L.sy + 1) >> 1;
		for (int it = begin + start; it < end; it += stride) {
			const int X = 2 * (it % bx) + (colour & 1), Y = 2 * ((it / bx) % by) + ((colour >> 1) & 1), Z = 2 * (it / (bx * by)) + (colour >> 2);
			if (X >= L.sx || Y >= L.sy || Z >= L.sz) continue;
			const int v = X + L.sx * (Y + L.sy * Z);
			if (L.t[v] == vtInactive) continue;
			const float sum = row27_sub<true>(L, v, X, Y, Z, L.b[v]);
			L.x[v] = sum / L.A[v];
		}
	}
}
MG_HD void pass_smooth(const Lv& L, bool l0, int colour, int start, int stride) { pass_smooth(L, l0, colour, 0, smooth_items(L, l0), start, stride); }
// knCalcResidual, multigrid.cpp:739-771
MG_HD void pass_residual(const Lv& L, bool l0, int begin, int end, int start, int stride) {
	for (int v = begin + start; v < end; v += stride) {
		if (L.t[v] == vtInactive) continue;
		const int X = v % L.sx, Y = (v / L.sx) % L.sy, Z = v / (L.sx * L.sy);
		float sum;
		if (l0) {
			sum = offdiag0(L, v, X, Y, Z, L.b[v]);
			sum -= L.A[v] * L.x[v];
		} else {
			sum = row27_sub<false>(L, v, X, Y, Z, L.b[v]);
		}
		L.r[v] = sum;
	}
}
MG_HD void pass_residual(const Lv& L, bool l0, int start, int stride) { pass_residual(L, l0, 0, L.n, start, stride); }
// knRestrict (b of the coarse level from r of the fine one), multigrid.cpp:904-927, and knSet(x_coarse, 0), :472
MG_HD void pass_restrict(const Lv& F, const Lv& C, int begin, int end, int start, int stride) {
	for (int idx = begin + start; idx < end; idx += stride) {
		C.x[idx] = 0.f;
		if (C.t[idx] == vtInactive) continue;
		const int VX = idx % C.sx, VY = (idx / C.sx) % C.sy, VZ = idx / (C.sx * C.sy);
		const int r0x = imax(0, VX * 2 - 1), r0y = imax(0, VY * 2 - 1), r0z = imax(0, VZ * 2 - 1);
		const int r1x = imin(F.sx - 1, VX * 2 + 1), r1y = imin(F.sy - 1, VY * 2 + 1), r1z = imin(F.sz - 1, VZ * 2 + 1);
		float sum = 0.f;
		for (int rz = r0z; rz <= r1z; rz++)
		for (int ry = r0y; ry <= r1y; ry++)
		for (int rx = r0x; rx <= r1x; rx++) {
			const int r = rx + F.sx * (ry + F.sy * rz);
			if (F.t[r] == vtInactive) continue;
			sum += pow2inv(odd3(rx, ry, rz)) * F.r[r];
		}
		C.b[idx] = sum;
	}
}
MG_HD void pass_restrict(const Lv& F, const Lv& C, int start, int stride) { pass_restrict(F, C, 0, C.n, start, stride); }
// knInterpolate into r of the fine level + knAddAssign(x, r), multigrid.cpp:484-486, 934-954.  The interpolated value is not
// stored: nothing reads r before the next residual pass overwrites it, and the inactive vertices (whose r stays 0) add 0.
MG_HD void pass_interp_add(const Lv& F, const Lv& C, int begin, int end, int start, int stride) {
	for (int v = begin + start; v < end; v += stride) {
		if (F.t[v] == vtInactive) continue;
		const int X = v % F.sx, Y = (v / F.sx) % F.sy, Z = v / (F.sx * F.sy);
		float sum = 0.f;
		for (int iz = Z / 2; iz <= (Z + 1) / 2; iz++)
		for (int iy = Y / 2; iy <= (Y + 1) / 2; iy++)
		for (int ix = X / 2; ix <= (X + 1) / 2; ix++) {
			const int i = ix + C.sx * (iy + C.sy * iz);
			if (C.t[i] != vtInactive) sum += C.x[i];
		}
		const float c = pow2inv(odd3(X, Y, Z)) * sum;
		F.x[v] = F.x[v] + c;
	}
}
MG_HD void pass_interp_add(const Lv& F, const Lv& C, int start, int stride) { pass_interp_add(F, C, 0, F.n, start, stride); }

// applyAStencil of solveCG (multigrid.cpp:798-826) on a double vector
MG_HD double cg_apply(const Lv& L, bool l0, int v, int X, int Y, int Z, const double* vec) {
	double sum = 0.0;
	if (l0) {
		const int py = L.sx, pz = L.sx * L.sy;
		const float *Ai = L.A + L.n, *Aj = L.A + 2 * L.n, *Ak = L.A + 3 * L.n;
		if (X > 0) sum += Ai[v - 1] * vec[v - 1];
		if (X < L.sx - 1) sum += Ai[v] * vec[v + 1];
		if (Y > 0) sum += Aj[v - py] * vec[v - py];
		if (Y < L.sy - 1) sum += Aj[v] * vec[v + py];
		if (Z > 0) sum += Ak[v - pz] * vec[v - pz];
		if (Z < L.sz - 1) sum += Ak[v] * vec[v + pz];
		sum += L.A[v] * vec[v];
	} else {
		int s = 0;
		for (int dz = -1; dz <= 1; dz++)
		for (int dy = -1; dy <= 1; dy++)
		for (int dx = -1; dx <= 1; dx++, s++) {
			const int nx = X + dx, ny = Y + dy, nz = Z + dz;
			if (nx < 0 || ny < 0 || nz < 0 || nx >= L.sx || ny >= L.sy || nz >= L.sz) continue;
			const int n = nx + L.sx * (ny + L.sy * nz);
			if (L.t[n] == vtInactive) continue;
			const float a = (s < 14) ? L.A[(13 - s) * L.n + n] : L.A[(s - 13) * L.n + v];
			sum += a * vec[n];
		}
	}
	return sum;
}

// ---------------------------------------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------------------------------------
// the level pyramid of GridMg::GridMg, multigrid.cpp:256-276: sizes ((s + 2) / 2 per axis); no further level once every axis
// is <= 5 or the level has <= 1000 vertices.  Returns the number of levels.
inline int pyramid(int sx, int sy, int sz, int (*sizes)[3]) {
	int nl = 0;
	for (int l = 0; l < MAXL; l++) {
		if (l > 0) {
			const int px = sizes[l - 1][0], py = sizes[l - 1][1], pz = sizes[l - 1][2];
			if ((px <= 5 && py <= 5 && pz <= 5) || px * py * pz <= 1000) break;      // multigrid.cpp:258-259
			sx = (px + 2) / 2;
			sy = (py + 2) / 2;
			sz = (pz + 2) / 2;
		}
		sizes[l][0] = sx;
		sizes[l][1] = sy;
		sizes[l][2] = sz;
		nl = l + 1;
	}
	return nl;
}

// the coarsening paths of level 1 in the reference's order, multigrid.cpp:286-318: generated U-major / stencil / N, then sorted by
// (sc, position of U) with std::sort -- the comparator leaves ties, and the operator sums in the resulting order, so the same
// generation order and the same algorithm are used here
inline std::vector<Path> make_paths() {
	static const int p7[7][3] = {{0, 0, 0}, {-1, 0, 0}, {1, 0, 0}, {0, -1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}};
	std::vector<Path> ps;
	for (int uz = 1; uz <= 3; uz++)
	for (int uy = 1; uy <= 3; uy++)
	for (int ux = 1; ux <= 3; ux++)
		for (int i = 0; i < 7; i++) {
			const int wx = ux + p7[i][0], wy = uy + p7[i][1], wz = uz + p7[i][2];
			for (int nz = wz / 2; nz <= (wz + 1) / 2; nz++)
			for (int ny = wy / 2; ny <= (wy + 1) / 2; ny++)
			for (int nx = wx / 2; nx <= (wx + 1) / 2; nx++) {
				const int s = nx + 3 * ny + 9 * nz;
				if (s < 13) continue;
				Path p;
				p.N[0] = nx - 1; p.N[1] = ny - 1; p.N[2] = nz - 1;
				p.U[0] = ux - 2; p.U[1] = uy - 2; p.U[2] = uz - 2;
				p.W[0] = wx - 2; p.W[1] = wy - 2; p.W[2] = wz - 2;
				p.sc = s - 13;
				p.sf = (i + 1) / 2;
				p.inU = (i % 2 == 0);
				p.rw = 1.f / float(1 << ((ux % 2) + (uy % 2) + (uz % 2)));
				p.iw = 1.f / float(1 << ((wx % 2) + (wy % 2) + (wz % 2)));
				ps.push_back(p);
			}
		}
	auto less = [](const Path& a, const Path& b) {
		if (a.sc == b.sc) return (a.U[0] + 1) + 3 * (a.U[1] + 1) + 9 * (a.U[2] + 1) < (b.U[0] + 1) + 3 * (b.U[1] + 1) + 9 * (b.U[2] + 1);
		return a.sc < b.sc;
	};
	std::sort(ps.begin(), ps.end(), less);
	return ps;
}

inline MgDim dim_of(const Lv& L) { return MgDim{L.sx, L.sy, L.sz, L.n}; }

// ---------------------------------------------------------------------------------------------------------
// what mgslab.hip (include/open/manta_hip_mgslab.h) borrows of a handle of mf_mg_create.  The registry of live handles and the
// kernels of the driver are multigrid.hip's own, so these three are defined there.  `who` is the entry name of the refusals.
// ---------------------------------------------------------------------------------------------------------
struct Borrowed {
	View v;              // the levels (device pointers of the handle; valid until mf_mg_destroy)
	int tail_first;      // first level of the single-workgroup tail
};
// refuses a destroyed or foreign handle (a 2-D one of mf_mg2d_create included) and a handle without a matrix, before reading it
int borrow(void* handle, const char* who, Borrowed* out);
// the levels 1 .. L-1 of a V-cycle, down and up again, exactly as mf_mg_vcycle queues them (grid-wide passes above the tail, the
// tail, grid-wide passes up to level 1); refuses a hierarchy whose tail holds level 0
int coarse_cycle(void* handle, const char* who, hipStream_t st);
// mCoarsestLevelAccuracy = accuracy * 1e-4, as InitPreconditionMultigrid sets it (conjugategrad.cpp:100-106)
int set_solve_accuracy(void* handle, const char* who, float accuracy);

}  // namespace mg3d
}  // namespace mf
