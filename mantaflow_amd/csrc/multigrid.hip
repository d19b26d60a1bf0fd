// multigrid.hip -- the multigrid preconditioner of the pressure PCG on gfx950 (include/manta_hip_multigrid.h).
// Reference: source/multigrid.{h,cpp} (GridMg, cited per kernel), source/conjugategrad.cpp:100-106, 162-167 (PC_MGP).
//
// Layout.  Level 0 keeps a private SoA copy of the 7-point stencil (planes A0, Ai, Aj, Ak; x fastest) because trivial rows
// are rescaled; levels > 0 keep the 14 stored entries of the symmetric 27-point stencil as 14 planes, so the 64 vertices of a
// wavefront read 14 coalesced streams.  Vertex types are one byte per vertex.
//
// Every pass of a V-cycle (a colour of the smoother, the residual, restriction, interpolation) is written once as a device
// function over "work items start, start + stride, ..." and used twice: by a grid-wide kernel (one item per thread) on the
// large levels, and by the single-workgroup tail kernel k_mg_tail, which runs every level of at most TAIL_VERTS vertices --
// down, the coarsest-level CG, and up again -- in ONE launch with workgroup barriers between the passes (below ~17^3 a pass is
// launch-bound).
//
// Set-up: the greedy coarse-vertex selection (genCoarseGrid) is serial and order-dependent; it runs on the host on the
// downloaded type bytes, with the reference's bucket heap order (mg_host.h, shared with the 2-D hierarchy of mg2d.hip).  Everything else of the set-up is a gather per vertex on the
// device.
#include "common.h"
#include "pressure.h"
#include "mg_host.h"
#include "../../include/manta_hip_multigrid.h"
#include <algorithm>
#include <chrono>
#include <vector>
#include <stdlib.h>
#include <string.h>

using namespace mf;

namespace {

constexpr int MAXL = 16;
constexpr int TAIL_BLOCK = 1024;      // one workgroup; the coarsest level has at most 1000 vertices (one per thread in the CG)
constexpr int TAIL_VERTS = 8192;      // levels of at most this many vertices run inside k_mg_tail
constexpr unsigned MG_MAGIC = 0x4d474d47u;

struct Lv {
	int sx, sy, sz, n;
	float* A;            // level 0: 4 planes of n; levels > 0: 14 planes of n
	float *x, *b, *r;
	unsigned char* t;
};
struct MgView {
	int nl;
	Lv l[MAXL];
};
// one precomputed coarsening path (V) <-restriction- (U) <-A_0- (W) <-interpolation- (N), multigrid.cpp:286-312
struct Path {
	signed char N[3], U[3], W[3];
	signed char sc, sf, inU;
	float rw, iw;
};

struct Mg {
	unsigned magic;
	int dev;
	MgView v;
	int nactive[MAXL];
	Path* paths;
	int npaths;
	int* d_info;          // [0] coarsest CG iterations of the last V-cycle, [1] non-zero stencil sum found, [2] trivial equations found
	bool aset;
	float coarsestAcc;    // mCoarsestLevelAccuracy
	int setups;
	int tail_first;
	int64_t us_host, us_dev;
};

__device__ __forceinline__ int odd3(int x, int y, int z) { return (x & 1) + (y & 1) + (z & 1); }
// 1 / (1 << k), k = 0..3: exact
__device__ __forceinline__ float pow2inv(int k) { return k == 0 ? 1.f : k == 1 ? 0.5f : k == 2 ? 0.25f : 0.125f; }

// ---------------------------------------------------------------------------------------------------------
// set-up
// ---------------------------------------------------------------------------------------------------------
// knCopyA + knActivateVertices + analyzeStencil, multigrid.cpp:321-384.  The reference scales the diagonal of trivial rows in
// place while other threads analyse their stencils; they only read the off-diagonals of their neighbours, which nobody changes.
__global__ void __launch_bounds__(BLOCK)
k_mg_copy_activate(Lv L, const float* __restrict__ A0, const float* __restrict__ Ai, const float* __restrict__ Aj, const float* __restrict__ Ak,
                   int* __restrict__ info) {
	const int v = blockIdx.x * BLOCK + threadIdx.x;
	if (v >= L.n) return;
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

// knGenCoarseGridOperator for l == 1, multigrid.cpp:594-614: the sorted paths, one after the other, into the 14 entries of V
__global__ void __launch_bounds__(BLOCK)
k_mg_operator1(Lv F, Lv C, const Path* __restrict__ paths, int npaths) {
	const int idx = blockIdx.x * BLOCK + threadIdx.x;
	if (idx >= C.n) return;
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
__global__ void __launch_bounds__(BLOCK)
k_mg_operatorN(Lv F, Lv C) {
	const int idx = blockIdx.x * BLOCK + threadIdx.x;
	if (idx >= C.n) return;
	if (C.t[idx] == vtInactive) return;
	const int VX = idx % C.sx, VY = (idx / C.sx) % C.sy, VZ = idx / (C.sx * C.sy);
	for (int s = 0; s < 14; s++) C.A[s * C.n + idx] = 0.f;
	const int u0x = max(0, VX * 2 - 1), u0y = max(0, VY * 2 - 1), u0z = max(0, VZ * 2 - 1);
	const int u1x = min(F.sx - 1, VX * 2 + 1), u1y = min(F.sy - 1, VY * 2 + 1), u1z = min(F.sz - 1, VZ * 2 + 1);
	for (int uz = u0z; uz <= u1z; uz++)
	for (int uy = u0y; uy <= u1y; uy++)
	for (int ux = u0x; ux <= u1x; ux++) {
		const int u = ux + F.sx * (uy + F.sy * uz);
		if (F.t[u] == vtInactive) continue;
		const float rw = pow2inv(odd3(ux, uy, uz));
		const int n1x = min(C.sx - 1, (ux + 2) / 2), n1y = min(C.sy - 1, (uy + 2) / 2), n1z = min(C.sz - 1, (uz + 2) / 2);
		for (int nz = (uz - 1) / 2; nz <= n1z; nz++)
		for (int ny = (uy - 1) / 2; ny <= n1y; ny++)
		for (int nx = (ux - 1) / 2; nx <= n1x; nx++) {
			const int nn = nx + C.sx * (ny + C.sy * nz);
			if (C.t[nn] == vtInactive) continue;
			const int sc = (nx - VX + 1) + 3 * (ny - VY + 1) + 9 * (nz - VZ + 1);
			if (sc < 13) continue;
			float* dstp = &C.A[(sc - 13) * C.n + idx];
			float acc = *dstp;
			const int w0x = max(0, max(ux - 1, nx * 2 - 1)), w0y = max(0, max(uy - 1, ny * 2 - 1)), w0z = max(0, max(uz - 1, nz * 2 - 1));
			const int w1x = min(F.sx - 1, min(ux + 1, nx * 2 + 1)), w1y = min(F.sy - 1, min(uy + 1, ny * 2 + 1)),
			          w1z = min(F.sz - 1, min(uz + 1, nz * 2 + 1));
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
// the passes of a V-cycle: device functions over the work items start, start + stride, ...
// ---------------------------------------------------------------------------------------------------------
// b - (off-diagonal part of A x) at vertex v of level 0 in knSmoothColor's / knCalcResidual's order, multigrid.cpp:684-689, 748-753
__device__ __forceinline__ float offdiag0(const Lv& L, int v, int X, int Y, int Z, float sum) {
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
// SKIP_CENTRE: the smoother leaves s == 13 out.  T is float (x) or double (the CG's vectors, with + instead of -).
template <bool SKIP_CENTRE>
__device__ __forceinline__ float row27_sub(const Lv& L, int v, int X, int Y, int Z, float sum) {
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

// knSmoothColor, multigrid.cpp:668-711, one colour.  Level 0: colour c is the parity (x + y + z) & 1 == c (the offsets
// {000, 110, 101, 011} and {100, 010, 001, 111}); an item is a pair of x-neighbours, of which one has the colour.  Levels > 0:
// colour c is the offset (c & 1, c >> 1 & 1, c >> 2) in the 2 x 2 x 2 blocks; an item is a block.  Vertices of one colour do
// not read each other.
__device__ __forceinline__ void pass_smooth(const Lv& L, bool l0, int colour, int start, int stride) {
	if (l0) {
		const int hx = (L.sx + 1) >> 1;
		const int items = hx * L.sy * L.sz;
		for (int it = start; it < items; it += stride) {
			const int q = it % hx, Y = (it / hx) % L.sy, Z = it / (hx * L.sy);
			const int X = 2 * q + ((Y + Z + colour) & 1);
			if (X >= L.sx) continue;
			const int v = X + L.sx * (Y + L.sy * Z);
			if (L.t[v] == vtInactive) continue;
			const float sum = offdiag0(L, v, X, Y, Z, L.b[v]);
			L.x[v] = sum / L.A[v];
		}
	} else {
		const int bx = (L.sx + 1) >> 1, by = (L.sy + 1) >> 1, bz = (L.sz + 1) >> 1;
		const int items = bx * by * bz;
		for (int it = start; it < items; it += stride) {
			const int X = 2 * (it % bx) + (colour & 1), Y = 2 * ((it / bx) % by) + ((colour >> 1) & 1), Z = 2 * (it / (bx * by)) + (colour >> 2);
			if (X >= L.sx || Y >= L.sy || Z >= L.sz) continue;
			const int v = X + L.sx * (Y + L.sy * Z);
			if (L.t[v] == vtInactive) continue;
			const float sum = row27_sub<true>(L, v, X, Y, Z, L.b[v]);
			L.x[v] = sum / L.A[v];
		}
	}
}
// knCalcResidual, multigrid.cpp:739-771
__device__ __forceinline__ void pass_residual(const Lv& L, bool l0, int start, int stride) {
	for (int v = start; v < L.n; v += stride) {
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
// knRestrict (b of the coarse level from r of the fine one), multigrid.cpp:904-927, and knSet(x_coarse, 0), :472
__device__ __forceinline__ void pass_restrict(const Lv& F, const Lv& C, int start, int stride) {
	for (int idx = start; idx < C.n; idx += stride) {
		C.x[idx] = 0.f;
		if (C.t[idx] == vtInactive) continue;
		const int VX = idx % C.sx, VY = (idx / C.sx) % C.sy, VZ = idx / (C.sx * C.sy);
		const int r0x = max(0, VX * 2 - 1), r0y = max(0, VY * 2 - 1), r0z = max(0, VZ * 2 - 1);
		const int r1x = min(F.sx - 1, VX * 2 + 1), r1y = min(F.sy - 1, VY * 2 + 1), r1z = min(F.sz - 1, VZ * 2 + 1);
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
// knInterpolate into r of the fine level + knAddAssign(x, r), multigrid.cpp:484-486, 934-954.  The interpolated value is not
// stored: nothing reads r before the next residual pass overwrites it, and the inactive vertices (whose r stays 0) add 0.
__device__ __forceinline__ void pass_interp_add(const Lv& F, const Lv& C, int start, int stride) {
	for (int v = start; v < F.n; v += stride) {
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

// grid-wide forms: one item per thread
__global__ void __launch_bounds__(BLOCK) k_mg_smooth(Lv L, int l0, int colour) {
	pass_smooth(L, l0 != 0, colour, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK);
}
__global__ void __launch_bounds__(BLOCK) k_mg_residual(Lv L, int l0) { pass_residual(L, l0 != 0, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK); }
__global__ void __launch_bounds__(BLOCK) k_mg_restrict(Lv F, Lv C) { pass_restrict(F, C, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK); }
__global__ void __launch_bounds__(BLOCK) k_mg_interp_add(Lv F, Lv C) { pass_interp_add(F, C, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK); }
// knSetRhs (trivial rows scaled), multigrid.cpp:417-424, and knSet(x_0, 0), :458
__global__ void __launch_bounds__(BLOCK) k_mg_set_rhs(Lv L, const float* __restrict__ rhs) {
	const int v = blockIdx.x * BLOCK + threadIdx.x;
	if (v >= L.n) return;
	float b = rhs[v];
	if (L.t[v] == vtActiveTrivial) b *= 1E-6f;
	L.b[v] = b;
	L.x[v] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------
// the tail: every level from `first` down, solveCG on the coarsest, and up again, in one workgroup
// ---------------------------------------------------------------------------------------------------------
// applyAStencil of solveCG (multigrid.cpp:798-826) on a double vector held in LDS
__device__ __forceinline__ double cg_apply(const Lv& L, bool l0, int v, int X, int Y, int Z, const double* vec) {
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
// the sum of a[0..n) in index order, as the reference's serial loop forms it (the entries of inactive vertices are +0, which
// leaves a sum that started at +0 unchanged)
__device__ __forceinline__ double ordered_sum(const double* a, int n) {
	double s = 0.0;
	int i = 0;
	for (; i + 8 <= n; i += 8) {
		const double a0 = a[i], a1 = a[i + 1], a2 = a[i + 2], a3 = a[i + 3], a4 = a[i + 4], a5 = a[i + 5], a6 = a[i + 6], a7 = a[i + 7];
		s += a0; s += a1; s += a2; s += a3; s += a4; s += a5; s += a6; s += a7;
	}
	for (; i < n; i++) s += a[i];
	return s;
}

__global__ void __launch_bounds__(TAIL_BLOCK)
k_mg_tail(MgView M, int first, float accuracy, int* __restrict__ info) {
	__shared__ double s_vec[TAIL_BLOCK];
	__shared__ double s_r1[TAIL_BLOCK];
	__shared__ double s_r2[TAIL_BLOCK];
	__shared__ double s_out[2];
	const int tid = threadIdx.x;
	const int last = M.nl - 1;
	// down, multigrid.cpp:460-475
	for (int l = first; l < last; l++) {
		const Lv& L = M.l[l];
		const int nc = (l == 0) ? 2 : 8;
		for (int c = 0; c < nc; c++) {
			pass_smooth(L, l == 0, c, tid, TAIL_BLOCK);
			__syncthreads();
		}
		pass_residual(L, l == 0, tid, TAIL_BLOCK);
		__syncthreads();
		pass_restrict(L, M.l[l + 1], tid, TAIL_BLOCK);
		__syncthreads();
	}
	// solveCG, multigrid.cpp:796-902: Jacobi-preconditioned CG in double, one vertex per thread, the three sums per iteration
	// in vertex order by one lane each
	{
		const Lv& L = M.l[last];
		const bool l0 = last == 0;
		const int v = tid;
		const bool in = v < L.n;
		const bool act = in && L.t[v] != vtInactive;
		const int X = in ? v % L.sx : 0, Y = in ? (v / L.sx) % L.sy : 0, Z = in ? v / (L.sx * L.sy) : 0;
		const float diag = act ? L.A[v] : 1.f;
		double x = in ? (double)L.x[v] : 0.0, r = 0.0, z = 0.0, p = 0.0;
		s_vec[tid] = x;
		__syncthreads();
		if (act) {
			r = L.b[v] - cg_apply(L, l0, v, X, Y, Z, s_vec);
			z = r / diag;
			p = z;
		}
		s_r1[tid] = act ? r * r : 0.0;
		s_r2[tid] = act ? r * z : 0.0;
		__syncthreads();
		if (tid == 0) s_out[0] = ordered_sum(s_r1, L.n);
		if (tid == 64) s_out[1] = ordered_sum(s_r2, L.n);
		__syncthreads();
		const double initialResidual = sqrt(s_out[0]);
		double alphaTop = s_out[1];
		int iter = 0;
		for (; iter < 10000 && initialResidual > 1E-12; iter++) {
			__syncthreads();
			s_vec[tid] = p;
			__syncthreads();
			if (act) z = cg_apply(L, l0, v, X, Y, Z, s_vec);
			s_r1[tid] = act ? p * z : 0.0;
			__syncthreads();
			if (tid == 0) s_out[0] = ordered_sum(s_r1, L.n);
			__syncthreads();
			const double alphaBot = s_out[0];
			const double alpha = alphaTop / alphaBot;
			if (act) {
				x += alpha * p;
				r -= alpha * z;
				z = r / diag;
			}
			__syncthreads();
			s_r1[tid] = act ? r * r : 0.0;
			s_r2[tid] = act ? r * z : 0.0;
			__syncthreads();
			if (tid == 0) s_out[0] = ordered_sum(s_r1, L.n);
			if (tid == 64) s_out[1] = ordered_sum(s_r2, L.n);
			__syncthreads();
			const double residual = sqrt(s_out[0]);
			const double alphaTopNew = s_out[1];
			if (residual / initialResidual < accuracy) break;
			const double beta = alphaTopNew / alphaTop;
			alphaTop = alphaTopNew;
			p = z + beta * p;
		}
		if (in) L.x[v] = (float)x;
		if (tid == 0) info[0] = iter;
		__syncthreads();
	}
	// up, multigrid.cpp:481-494 (colours in reversed order)
	for (int l = last - 1; l >= first; l--) {
		const Lv& L = M.l[l];
		pass_interp_add(L, M.l[l + 1], tid, TAIL_BLOCK);
		__syncthreads();
		const int nc = (l == 0) ? 2 : 8;
		for (int c = nc - 1; c >= 0; c--) {
			pass_smooth(L, l == 0, c, tid, TAIL_BLOCK);
			__syncthreads();
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
// the handles that mf_mg_create gave out and mf_mg_destroy has not taken back (mg_host.h)
LiveHandles g_live;
Mg* as_mg(void* h) {
	if (!h || !g_live.has(h)) return nullptr;
	Mg* m = (Mg*)h;
	return m->magic == MG_MAGIC ? m : nullptr;
}
MgDim dim_of(const Lv& L) { return MgDim{L.sx, L.sy, L.sz, L.n}; }

// the coarsening paths of level 1 in the reference's order, multigrid.cpp:286-318: generated U-major / stencil / N, then sorted by
// (sc, position of U) with std::sort -- the comparator leaves ties, and the operator sums in the resulting order, so the same
// generation order and the same algorithm are used here
std::vector<Path> make_paths() {
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

void free_levels(Mg* m) {
	for (int l = 0; l < m->v.nl; l++) {
		Lv& L = m->v.l[l];
		(void)hipFree(L.A);
		(void)hipFree(L.x);
		(void)hipFree(L.b);
		(void)hipFree(L.r);
		(void)hipFree(L.t);
	}
	(void)hipFree(m->paths);
	(void)hipFree(m->d_info);
}

int mg_set_a(Mg* m, const float* A0, const float* Ai, const float* Aj, const float* Ak, hipStream_t st) {
	using clk = std::chrono::steady_clock;
	const auto t0 = clk::now();
	int64_t us_host = 0;
	MgView& V = m->v;
	MF_HIP(hipMemsetAsync(m->d_info, 0, 3 * sizeof(int), st));
	hipLaunchKernelGGL(k_mg_copy_activate, dim3(nblk(V.l[0].n)), dim3(BLOCK), 0, st, V.l[0], A0, Ai, Aj, Ak, m->d_info);
	MF_LAUNCH_CHECK();
	std::vector<unsigned char> tf(V.l[0].n), tc;
	MF_HIP(hipMemcpyAsync(tf.data(), V.l[0].t, tf.size(), hipMemcpyDeviceToHost, st));
	MF_HIP(hipStreamSynchronize(st));
	int act = 0;
	for (unsigned char c : tf) act += c != vtInactive;
	m->nactive[0] = act;
	for (int l = 1; l < V.nl; l++) {
		const auto h0 = clk::now();
		tc.resize(V.l[l].n);
		m->nactive[l] = select_coarse(dim_of(V.l[l - 1]), tf.data(), dim_of(V.l[l]), tc.data());
		us_host += std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - h0).count();
		MF_HIP(hipMemcpyAsync(V.l[l].t, tc.data(), tc.size(), hipMemcpyHostToDevice, st));
		if (l == 1) hipLaunchKernelGGL(k_mg_operator1, dim3(nblk(V.l[l].n)), dim3(BLOCK), 0, st, V.l[0], V.l[1], m->paths, m->npaths);
		else hipLaunchKernelGGL(k_mg_operatorN, dim3(nblk(V.l[l].n)), dim3(BLOCK), 0, st, V.l[l - 1], V.l[l]);
		MF_LAUNCH_CHECK();
		MF_HIP(hipStreamSynchronize(st));      // tc is reused by the next level
		tf.swap(tc);
	}
	MF_HIP(hipStreamSynchronize(st));
	m->aset = true;
	m->setups++;
	m->us_host = us_host;
	m->us_dev = std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - t0).count() - us_host;
	return 0;
}

int mg_vcycle(Mg* m, float* dst, const float* rhs, hipStream_t st) {
	if (!m->aset) return fail("mf_mg_vcycle: GridMg::setRhs Error: A has not been set.");
	const MgView& V = m->v;
	const int first = m->tail_first;
	hipLaunchKernelGGL(k_mg_set_rhs, dim3(nblk(V.l[0].n)), dim3(BLOCK), 0, st, V.l[0], rhs);
	for (int l = 0; l < first; l++) {
		const Lv& L = V.l[l];
		const int l0 = l == 0;
		const int items = l0 ? ((L.sx + 1) / 2) * L.sy * L.sz : ((L.sx + 1) / 2) * ((L.sy + 1) / 2) * ((L.sz + 1) / 2);
		for (int c = 0; c < (l0 ? 2 : 8); c++) hipLaunchKernelGGL(k_mg_smooth, dim3(nblk(items)), dim3(BLOCK), 0, st, L, l0, c);
		hipLaunchKernelGGL(k_mg_residual, dim3(nblk(L.n)), dim3(BLOCK), 0, st, L, l0);
		hipLaunchKernelGGL(k_mg_restrict, dim3(nblk(V.l[l + 1].n)), dim3(BLOCK), 0, st, L, V.l[l + 1]);
	}
	hipLaunchKernelGGL(k_mg_tail, dim3(1), dim3(TAIL_BLOCK), 0, st, V, first, m->coarsestAcc, m->d_info);
	for (int l = first - 1; l >= 0; l--) {
		const Lv& L = V.l[l];
		const int l0 = l == 0;
		const int items = l0 ? ((L.sx + 1) / 2) * L.sy * L.sz : ((L.sx + 1) / 2) * ((L.sy + 1) / 2) * ((L.sz + 1) / 2);
		hipLaunchKernelGGL(k_mg_interp_add, dim3(nblk(L.n)), dim3(BLOCK), 0, st, L, V.l[l + 1]);
		for (int c = (l0 ? 2 : 8) - 1; c >= 0; c--) hipLaunchKernelGGL(k_mg_smooth, dim3(nblk(items)), dim3(BLOCK), 0, st, L, l0, c);
	}
	MF_LAUNCH_CHECK();
	MF_HIP(hipMemcpyAsync(dst, V.l[0].x, sizeof(float) * V.l[0].n, hipMemcpyDeviceToDevice, st));      // knCopyToGrid, multigrid.cpp:499
	return 0;
}

int ext_init(void* ctx, const float* A0, const float* Ai, const float* Aj, const float* Ak, float accuracy, hipStream_t st) {
	Mg* m = (Mg*)ctx;
	if (!m->aset) MF_TRY(mg_set_a(m, A0, Ai, Aj, Ak, st));      // InitPreconditionMultigrid, conjugategrad.cpp:100-106
	m->coarsestAcc = (float)(accuracy * 1E-4);
	return 0;
}
int ext_apply(void* ctx, float* dst, const float* src, hipStream_t st) { return mg_vcycle((Mg*)ctx, dst, src, st); }

}  // namespace

extern "C" {

int mf_multigrid_abi_version(void) { return MF_MULTIGRID_ABI_VERSION; }

int mf_mg_create(int sx, int sy, int sz, void** handle_out) {
	if (!handle_out) return fail("mf_mg_create: null handle_out");
	*handle_out = nullptr;
	MF_TRY(check_dim(sx, sy, sz));
	if (sz <= 1) return fail("mf_mg_create: 2-D grids are not supported by the multigrid preconditioner on this backend (3-D only)");
	Mg* m = new Mg();
	m->magic = MG_MAGIC;
	m->coarsestAcc = 1E-8f;
	MF_HIP(hipGetDevice(&m->dev));
	MgView& V = m->v;
	int s[3] = {sx, sy, sz};
	int rc = 0;
	for (int l = 0; l < MAXL; l++) {
		if (l > 0) {
			const Lv& P = V.l[l - 1];
			if ((P.sx <= 5 && P.sy <= 5 && P.sz <= 5) || P.n <= 1000) break;      // multigrid.cpp:258-259
			s[0] = (P.sx + 2) / 2;
			s[1] = (P.sy + 2) / 2;
			s[2] = (P.sz + 2) / 2;
		}
		Lv& L = V.l[l];
		L.sx = s[0];
		L.sy = s[1];
		L.sz = s[2];
		L.n = s[0] * s[1] * s[2];
		const size_t na = (size_t)L.n * (l == 0 ? 4 : 14) * sizeof(float), nv = (size_t)L.n * sizeof(float);
		V.nl = l + 1;
		hipError_t e = hipMalloc((void**)&L.A, na);
		if (e == hipSuccess) e = hipMalloc((void**)&L.x, nv);
		if (e == hipSuccess) e = hipMalloc((void**)&L.b, nv);
		if (e == hipSuccess) e = hipMalloc((void**)&L.r, nv);
		if (e == hipSuccess) e = hipMalloc((void**)&L.t, (size_t)L.n);
		if (e == hipSuccess) e = hipMemset(L.A, 0, na);
		if (e == hipSuccess) e = hipMemset(L.x, 0, nv);
		if (e == hipSuccess) e = hipMemset(L.b, 0, nv);
		if (e == hipSuccess) e = hipMemset(L.r, 0, nv);
		if (e == hipSuccess) e = hipMemset(L.t, 0, (size_t)L.n);
		if (e != hipSuccess) {
			rc = fail("mf_mg_create: level %d (%d x %d x %d): %s", l, L.sx, L.sy, L.sz, hipGetErrorString(e));
			break;
		}
	}
	if (rc == 0 && V.l[V.nl - 1].n > TAIL_BLOCK) rc = fail("mf_mg_create: coarsest level has %d vertices (at most %d supported)", V.l[V.nl - 1].n, TAIL_BLOCK);
	if (rc == 0) {
		const std::vector<Path> ps = make_paths();
		m->npaths = (int)ps.size();
		hipError_t e = hipMalloc((void**)&m->paths, ps.size() * sizeof(Path));
		if (e == hipSuccess) e = hipMemcpy(m->paths, ps.data(), ps.size() * sizeof(Path), hipMemcpyHostToDevice);
		if (e == hipSuccess) e = hipMalloc((void**)&m->d_info, 4 * sizeof(int));
		if (e == hipSuccess) e = hipMemset(m->d_info, 0, 4 * sizeof(int));
		if (e != hipSuccess) rc = fail("mf_mg_create: %s", hipGetErrorString(e));
	}
	if (rc != 0) {
		(void)hipGetLastError();
		free_levels(m);
		m->magic = 0;
		delete m;
		return rc;
	}
	// the single-workgroup tail takes every level of at most TAIL_VERTS vertices, and always the coarsest (MF_MG_TAIL_VERTS: a
	// measurement knob -- 0 leaves the tail the coarsest-level CG alone; the results do not depend on it)
	int tail_verts = TAIL_VERTS;
	if (const char* e = getenv("MF_MG_TAIL_VERTS")) tail_verts = atoi(e);
	m->tail_first = V.nl - 1;
	while (m->tail_first > 0 && V.l[m->tail_first - 1].n <= tail_verts) m->tail_first--;
	g_live.insert(m);
	*handle_out = m;
	return 0;
}

int mf_mg_destroy(void* handle) {
	Mg* m = as_mg(handle);
	if (!m) return fail("mf_mg_destroy: bad handle");
	MF_HIP(hipDeviceSynchronize());
	g_live.erase(handle);
	free_levels(m);
	m->magic = 0;
	delete m;
	return 0;
}

int mf_mg_set_a(void* handle, const float* A0, const float* Ai, const float* Aj, const float* Ak, void* stream) {
	Mg* m = as_mg(handle);
	if (!m) return fail("mf_mg_set_a: bad handle");
	return mg_set_a(m, A0, Ai, Aj, Ak, (hipStream_t)stream);
}

int mf_mg_is_a_set(void* handle) {
	Mg* m = as_mg(handle);
	return m ? (m->aset ? 1 : 0) : -1;
}

int mf_mg_vcycle(void* handle, float* dst, const float* rhs, void* stream) {
	Mg* m = as_mg(handle);
	if (!m) return fail("mf_mg_vcycle: bad handle");
	return mg_vcycle(m, dst, rhs, (hipStream_t)stream);
}

int mf_mg_cg_solve(void* handle, int sx, int sy, int sz, const int32_t* flags, float* dst, const float* rhs, float* residual,
                   float* search, float* tmp, const float* A0, const float* Ai, const float* Aj, const float* Ak, float accuracy,
                   int maxIter, int useL2Norm, float* out_host, void* stream) {
	Mg* m = as_mg(handle);
	if (!m) return fail("mf_mg_cg_solve: bad handle");
	MF_TRY(check_dim(sx, sy, sz));
	const Lv& L0 = m->v.l[0];
	if (sx != L0.sx || sy != L0.sy || sz != L0.sz)
		return fail("mf_mg_cg_solve: the hierarchy was created for %d x %d x %d, the system is %d x %d x %d", L0.sx, L0.sy, L0.sz, sx, sy, sz);
	const Dim d = mkdim(sx, sy, sz);
	PcExternal ext = {ext_init, ext_apply, m};
	return cg_solve_external(d, flags, dst, rhs, residual, search, tmp, A0, Ai, Aj, Ak, &ext, accuracy, maxIter, useL2Norm, out_host, stream);
}

int mf_mg_info(void* handle, int64_t* out_host, int n_out) {
	Mg* m = as_mg(handle);
	if (!m) return fail("mf_mg_info: bad handle");
	if (n_out < 8 + 4 * m->v.nl) return fail("mf_mg_info: out_host holds %d entries, %d needed", n_out, 8 + 4 * m->v.nl);
	int info[3] = {0, 0, 0};
	MF_HIP(hipDeviceSynchronize());
	MF_HIP(hipMemcpy(info, m->d_info, sizeof info, hipMemcpyDeviceToHost));
	out_host[0] = m->v.nl;
	out_host[1] = m->setups;
	out_host[2] = info[0];
	out_host[3] = info[1];
	out_host[4] = info[2];
	out_host[5] = m->tail_first;
	out_host[6] = m->us_host;
	out_host[7] = m->us_dev;
	for (int l = 0; l < m->v.nl; l++) {
		out_host[8 + 4 * l] = m->v.l[l].sx;
		out_host[9 + 4 * l] = m->v.l[l].sy;
		out_host[10 + 4 * l] = m->v.l[l].sz;
		out_host[11 + 4 * l] = m->aset ? m->nactive[l] : 0;
	}
	return 0;
}

int mf_mg_read_level(void* handle, int level, int what, void* dst_host, int64_t bytes) {
	Mg* m = as_mg(handle);
	if (!m) return fail("mf_mg_read_level: bad handle");
	if (level < 0 || level >= m->v.nl) return fail("mf_mg_read_level: level %d of %d", level, m->v.nl);
	const Lv& L = m->v.l[level];
	const void* src;
	int64_t want;
	switch (what) {
		case 0: src = L.t; want = L.n; break;
		case 1: src = L.A; want = (int64_t)L.n * (level == 0 ? 4 : 14) * sizeof(float); break;
		case 2: src = L.x; want = (int64_t)L.n * sizeof(float); break;
		case 3: src = L.b; want = (int64_t)L.n * sizeof(float); break;
		default: return fail("mf_mg_read_level: what = %d", what);
	}
	if (bytes != want) return fail("mf_mg_read_level: %lld bytes given, the array has %lld", (long long)bytes, (long long)want);
	MF_HIP(hipDeviceSynchronize());
	MF_HIP(hipMemcpy(dst_host, src, (size_t)want, hipMemcpyDeviceToHost));
	return 0;
}

}  // extern "C"
