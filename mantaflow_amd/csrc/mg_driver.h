// mg_driver.h -- everything of the multigrid preconditioner that does not depend on the dimension, once, as templates over a
// description H of a hierarchy: the handle, the kernels (the grid-wide wrappers and the single-workgroup tail with the
// coarsest-level CG), set-up, V-cycle and the bodies of the C entries.  multigrid.hip instantiates it with the 3-D hierarchy
// (mg3d_cells.h) and mg2d.hip with the 2-D one (mg2d_cells.h); the choice is made at compile time only.
// Reference: source/multigrid.{h,cpp} (GridMg), source/conjugategrad.cpp:100-106, 162-167 (PC_MGP).
//
// H supplies what differs between the dimensions:
//   Lv, View, Path, Coord            the level (its layout is H's own), the levels of a handle as a kernel argument, a coarsening
//                                    path, the coordinates of a vertex
//   MAGIC, NAME                      the word in a live handle; the entry-name prefix of the messages ("mf_mg", "mf_mg2d")
//   check_create(sx, sy, sz)         a refusal of H's own at create, after the common ones
//   pyramid(sx, sy, sz, Lv*)         sx, sy (, sz), n of every level -> the number of levels
//   size_str(MgDim)                  a level's size as the messages print it ("11 x 10 x 10", "33 x 31")
//   planes(l0), smooth_colours(l0)   the stencil planes a level stores; the colours of its smoother
//   make_paths()                     the sorted paths of operator1
//   coord(L, v), cg_apply(L, l0, v, coord, vec), copy_activate(L, v, A0, Ai, Aj, Ak, info)
// and, in the namespace of H::Lv (mg3d_cells.h, mg2d_cells.h), the per-vertex bodies that take a level and are called here by
// their plain names, so that the overload for H::Lv is the one chosen:
//   operator1, operatorN, smooth_items, pass_smooth, pass_residual, pass_restrict, pass_interp_add, dim_of
//
// Every pass of a V-cycle (a colour of the smoother, the residual, restriction, interpolation) is a function of H over "work
// items start, start + stride, ..." and is used twice: by a grid-wide kernel (one item per thread) on the large levels, and by
// the single-workgroup tail kernel k_mg_tail, which runs every level of at most TAIL_VERTS vertices -- down, the coarsest-level
// CG, and up again -- in ONE launch with workgroup barriers between the passes (below ~17^3 a pass is launch-bound; a 2-D
// pyramid is deeper than a 3-D one of the same cell count, and the tail takes 9 launches per level away).
//
// Set-up: the greedy coarse-vertex selection (genCoarseGrid) is serial and order-dependent; it runs on the host on the
// downloaded type bytes, with the reference's bucket heap order (mg_host.h).  Everything else of the set-up is a gather per
// vertex on the device.
//
// Everything here is in an unnamed namespace: the kernels and the registry of live handles are the including file's own.
#pragma once
#include "common.h"
#include "pressure.h"
#include "mg_host.h"
#include <chrono>
#include <stdlib.h>
#include <vector>

namespace mf {
namespace {

constexpr int TAIL_BLOCK = 1024;      // one workgroup; the coarsest level has at most 1000 vertices (one per thread in the CG)
constexpr int TAIL_VERTS = 8192;      // levels of at most this many vertices run inside k_mg_tail

// a level's size as text (H::size_str)
struct SizeStr {
	char s[48];
};

template <class H>
struct Mg {
	unsigned magic;
	int dev;
	typename H::View v;
	int nactive[MAXL];
	typename H::Path* paths;
	int npaths;
	int* d_info;          // [0] coarsest CG iterations of the last V-cycle, [1] non-zero stencil sum found, [2] trivial equations found
	bool aset;
	float coarsestAcc;    // mCoarsestLevelAccuracy
	int setups;
	int tail_first;
	int64_t us_host, us_dev;
};

// ---------------------------------------------------------------------------------------------------------
// grid-wide forms: one item per thread
// ---------------------------------------------------------------------------------------------------------
template <class H>
__global__ void __launch_bounds__(BLOCK)
k_mg_copy_activate(typename H::Lv L, const float* __restrict__ A0, const float* __restrict__ Ai, const float* __restrict__ Aj, const float* __restrict__ Ak,
                   int* __restrict__ info) {
	const int v = blockIdx.x * BLOCK + threadIdx.x;
	if (v < L.n) H::copy_activate(L, v, A0, Ai, Aj, Ak, info);
}
template <class H>
__global__ void __launch_bounds__(BLOCK) k_mg_operator1(typename H::Lv F, typename H::Lv C, const typename H::Path* __restrict__ paths, int npaths) {
	const int idx = blockIdx.x * BLOCK + threadIdx.x;
	if (idx < C.n) operator1(F, C, idx, paths, npaths);
}
template <class H>
__global__ void __launch_bounds__(BLOCK) k_mg_operatorN(typename H::Lv F, typename H::Lv C) {
	const int idx = blockIdx.x * BLOCK + threadIdx.x;
	if (idx < C.n) operatorN(F, C, idx);
}
template <class H>
__global__ void __launch_bounds__(BLOCK) k_mg_smooth(typename H::Lv L, int l0, int colour) {
	pass_smooth(L, l0 != 0, colour, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK);
}
template <class H>
__global__ void __launch_bounds__(BLOCK) k_mg_residual(typename H::Lv L, int l0) {
	pass_residual(L, l0 != 0, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK);
}
template <class H>
__global__ void __launch_bounds__(BLOCK) k_mg_restrict(typename H::Lv F, typename H::Lv C) {
	pass_restrict(F, C, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK);
}
template <class H>
__global__ void __launch_bounds__(BLOCK) k_mg_interp_add(typename H::Lv F, typename H::Lv C) {
	pass_interp_add(F, C, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK);
}
template <class H>
__global__ void __launch_bounds__(BLOCK) k_mg_set_rhs(typename H::Lv L, const float* __restrict__ rhs) {
	const int v = blockIdx.x * BLOCK + threadIdx.x;
	if (v < L.n) set_rhs(L, v, rhs);
}

// ---------------------------------------------------------------------------------------------------------
// the tail: every level from `first` down, solveCG on the coarsest, and up again, in one workgroup
// ---------------------------------------------------------------------------------------------------------
template <class H>
__global__ void __launch_bounds__(TAIL_BLOCK)
k_mg_tail(typename H::View M, int first, float accuracy, int* __restrict__ info) {
	using Lv = typename H::Lv;
	__shared__ double s_vec[TAIL_BLOCK];
	__shared__ double s_r1[TAIL_BLOCK];
	__shared__ double s_r2[TAIL_BLOCK];
	__shared__ double s_out[2];
	const int tid = threadIdx.x;
	const int last = M.nl - 1;
	// down, multigrid.cpp:460-475
	for (int l = first; l < last; l++) {
		const Lv& L = M.l[l];
		for (int c = 0; c < H::smooth_colours(l == 0); c++) {
			pass_smooth(L, l == 0, c, tid, TAIL_BLOCK);
			__syncthreads();
		}
		pass_residual(L, l == 0, tid, TAIL_BLOCK);
		__syncthreads();
		pass_restrict(L, M.l[l + 1], tid, TAIL_BLOCK);
		__syncthreads();
	}
	// solveCG, multigrid.cpp:796-902: Jacobi-preconditioned CG in double, one vertex per thread, the three sums per iteration
	// in vertex order by one lane each; applyAStencil (H::cg_apply) reads the vector from LDS
	{
		const Lv& L = M.l[last];
		const bool l0 = last == 0;
		const int v = tid;
		const bool in = v < L.n;
		const bool act = in && L.t[v] != vtInactive;
		const typename H::Coord at = in ? H::coord(L, v) : typename H::Coord{};
		const float diag = act ? L.A[v] : 1.f;
		double x = in ? (double)L.x[v] : 0.0, r = 0.0, z = 0.0, p = 0.0;
		s_vec[tid] = x;
		__syncthreads();
		if (act) {
			r = L.b[v] - H::cg_apply(L, l0, v, at, s_vec);
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
			if (act) z = H::cg_apply(L, l0, v, at, s_vec);
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
		for (int c = H::smooth_colours(l == 0) - 1; c >= 0; c--) {
			pass_smooth(L, l == 0, c, tid, TAIL_BLOCK);
			__syncthreads();
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
// the handles that H's create entry gave out and its destroy entry has not taken back (mg_host.h): one registry per hierarchy,
// so a handle of the other kind is a bad handle
template <class H>
LiveHandles g_live;
template <class H>
Mg<H>* as_mg(void* h) {
	if (!h || !g_live<H>.has(h)) return nullptr;
	Mg<H>* m = (Mg<H>*)h;
	return m->magic == H::MAGIC ? m : nullptr;
}

template <class H>
void free_levels(Mg<H>* m) {
	for (int l = 0; l < m->v.nl; l++) {
		typename H::Lv& L = m->v.l[l];
		(void)hipFree(L.A);
		(void)hipFree(L.x);
		(void)hipFree(L.b);
		(void)hipFree(L.r);
		(void)hipFree(L.t);
	}
	(void)hipFree(m->paths);
	(void)hipFree(m->d_info);
}

// the four planes the PCG hands over; a 2-D system has no Ak and its copy_activate does not look at it
template <class H>
int set_a(Mg<H>* m, const float* A0, const float* Ai, const float* Aj, const float* Ak, hipStream_t st) {
	using clk = std::chrono::steady_clock;
	const auto t0 = clk::now();
	int64_t us_host = 0;
	typename H::View& V = m->v;
	MF_HIP(hipMemsetAsync(m->d_info, 0, 3 * sizeof(int), st));
	hipLaunchKernelGGL(k_mg_copy_activate<H>, dim3(nblk(V.l[0].n)), dim3(BLOCK), 0, st, V.l[0], A0, Ai, Aj, Ak, m->d_info);
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
		if (l == 1) hipLaunchKernelGGL(k_mg_operator1<H>, dim3(nblk(V.l[l].n)), dim3(BLOCK), 0, st, V.l[0], V.l[1], m->paths, m->npaths);
		else hipLaunchKernelGGL(k_mg_operatorN<H>, dim3(nblk(V.l[l].n)), dim3(BLOCK), 0, st, V.l[l - 1], V.l[l]);
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

// the levels from .. L-1 of doVCycle, down and up again (multigrid.cpp:460-494): grid-wide passes on the levels above the tail,
// the tail, grid-wide passes back up to level `from`.  from <= tail_first; a whole V-cycle is from = 0, and a caller that has
// done level 0 itself (mgslab.hip, on a range of planes per rank) runs from = 1 between its restriction and its interpolation.
template <class H>
void levels_down_up(Mg<H>* m, int from, hipStream_t st) {
	using Lv = typename H::Lv;
	const typename H::View& V = m->v;
	const int first = m->tail_first;
	for (int l = from; l < first; l++) {
		const Lv& L = V.l[l];
		const int l0 = l == 0;
		const int items = smooth_items(L, l0);
		for (int c = 0; c < H::smooth_colours(l0); c++) hipLaunchKernelGGL(k_mg_smooth<H>, dim3(nblk(items)), dim3(BLOCK), 0, st, L, l0, c);
		hipLaunchKernelGGL(k_mg_residual<H>, dim3(nblk(L.n)), dim3(BLOCK), 0, st, L, l0);
		hipLaunchKernelGGL(k_mg_restrict<H>, dim3(nblk(V.l[l + 1].n)), dim3(BLOCK), 0, st, L, V.l[l + 1]);
	}
	hipLaunchKernelGGL(k_mg_tail<H>, dim3(1), dim3(TAIL_BLOCK), 0, st, V, first, m->coarsestAcc, m->d_info);
	for (int l = first - 1; l >= from; l--) {
		const Lv& L = V.l[l];
		const int l0 = l == 0;
		const int items = smooth_items(L, l0);
		hipLaunchKernelGGL(k_mg_interp_add<H>, dim3(nblk(L.n)), dim3(BLOCK), 0, st, L, V.l[l + 1]);
		for (int c = H::smooth_colours(l0) - 1; c >= 0; c--) hipLaunchKernelGGL(k_mg_smooth<H>, dim3(nblk(items)), dim3(BLOCK), 0, st, L, l0, c);
	}
}

template <class H>
int vcycle(Mg<H>* m, float* dst, const float* rhs, hipStream_t st) {
	if (!m->aset) return fail("%s_vcycle: GridMg::setRhs Error: A has not been set.", H::NAME);
	const typename H::View& V = m->v;
	hipLaunchKernelGGL(k_mg_set_rhs<H>, dim3(nblk(V.l[0].n)), dim3(BLOCK), 0, st, V.l[0], rhs);
	levels_down_up(m, 0, st);
	MF_LAUNCH_CHECK();
	MF_HIP(hipMemcpyAsync(dst, V.l[0].x, sizeof(float) * V.l[0].n, hipMemcpyDeviceToDevice, st));      // knCopyToGrid, multigrid.cpp:499
	return 0;
}

template <class H>
int ext_init(void* ctx, const float* A0, const float* Ai, const float* Aj, const float* Ak, float accuracy, hipStream_t st) {
	Mg<H>* m = (Mg<H>*)ctx;
	if (!m->aset) MF_TRY(set_a(m, A0, Ai, Aj, Ak, st));      // InitPreconditionMultigrid, conjugategrad.cpp:100-106
	m->coarsestAcc = (float)(accuracy * 1E-4);
	return 0;
}
template <class H>
int ext_apply(void* ctx, float* dst, const float* src, hipStream_t st) {
	return vcycle((Mg<H>*)ctx, dst, src, st);
}

// ---------------------------------------------------------------------------------------------------------
// the bodies of the C entries (a 2-D entry passes sz = 1 and Ak = nullptr)
// ---------------------------------------------------------------------------------------------------------
template <class H>
int mg_create(int sx, int sy, int sz, void** handle_out) {
	using Lv = typename H::Lv;
	using Path = typename H::Path;
	if (!handle_out) return fail("%s_create: null handle_out", H::NAME);
	*handle_out = nullptr;
	MF_TRY(check_dim(sx, sy, sz));
	MF_TRY(H::check_create(sx, sy, sz));
	Mg<H>* m = new Mg<H>();
	m->magic = H::MAGIC;
	m->coarsestAcc = 1E-8f;
	MF_HIP(hipGetDevice(&m->dev));
	typename H::View& V = m->v;
	const int nl = H::pyramid(sx, sy, sz, V.l);
	int rc = 0;
	for (int l = 0; l < nl; l++) {
		Lv& L = V.l[l];
		const size_t na = (size_t)L.n * H::planes(l == 0) * sizeof(float), nv = (size_t)L.n * sizeof(float);
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
			rc = fail("%s_create: level %d (%s): %s", H::NAME, l, H::size_str(dim_of(L)).s, hipGetErrorString(e));
			break;
		}
	}
	// (the pyramid rule leaves at most 1000 vertices on the last level unless MAXL levels did not reach it)
	if (rc == 0 && V.l[V.nl - 1].n > TAIL_BLOCK)
		rc = fail("%s_create: coarsest level has %d vertices (at most %d supported)", H::NAME, V.l[V.nl - 1].n, TAIL_BLOCK);
	if (rc == 0) {
		const std::vector<Path> ps = H::make_paths();
		m->npaths = (int)ps.size();
		hipError_t e = hipMalloc((void**)&m->paths, ps.size() * sizeof(Path));
		if (e == hipSuccess) e = hipMemcpy(m->paths, ps.data(), ps.size() * sizeof(Path), hipMemcpyHostToDevice);
		if (e == hipSuccess) e = hipMalloc((void**)&m->d_info, 4 * sizeof(int));
		if (e == hipSuccess) e = hipMemset(m->d_info, 0, 4 * sizeof(int));
		// create has no stream: its fills are done before it returns, so a caller's stream of any kind finds the levels cleared
		if (e == hipSuccess) e = hipDeviceSynchronize();
		if (e != hipSuccess) rc = fail("%s_create: %s", H::NAME, hipGetErrorString(e));
	}
	if (rc != 0) {
		(void)hipGetLastError();
		free_levels(m);
		m->magic = 0;
		delete m;
		return rc;
	}
	// the single-workgroup tail takes every level of at most TAIL_VERTS vertices, and always the coarsest (MF_MG_TAIL_VERTS: a
	// measurement knob of both hierarchies -- 0 leaves the tail the coarsest-level CG alone; the results do not depend on it)
	int tail_verts = TAIL_VERTS;
	if (const char* e = getenv("MF_MG_TAIL_VERTS")) tail_verts = atoi(e);
	m->tail_first = V.nl - 1;
	while (m->tail_first > 0 && V.l[m->tail_first - 1].n <= tail_verts) m->tail_first--;
	g_live<H>.insert(m);
	*handle_out = m;
	return 0;
}

template <class H>
int mg_destroy(void* handle) {
	Mg<H>* m = as_mg<H>(handle);
	if (!m) return fail("%s_destroy: bad handle", H::NAME);
	MF_HIP(hipDeviceSynchronize());
	g_live<H>.erase(handle);
	free_levels(m);
	m->magic = 0;
	delete m;
	return 0;
}

template <class H>
int mg_set_a(void* handle, const float* A0, const float* Ai, const float* Aj, const float* Ak, void* stream) {
	Mg<H>* m = as_mg<H>(handle);
	if (!m) return fail("%s_set_a: bad handle", H::NAME);
	return set_a(m, A0, Ai, Aj, Ak, (hipStream_t)stream);
}

template <class H>
int mg_is_a_set(void* handle) {
	Mg<H>* m = as_mg<H>(handle);
	return m ? (m->aset ? 1 : 0) : -1;
}

template <class H>
int mg_vcycle(void* handle, float* dst, const float* rhs, void* stream) {
	Mg<H>* m = as_mg<H>(handle);
	if (!m) return fail("%s_vcycle: bad handle", H::NAME);
	return vcycle(m, dst, rhs, (hipStream_t)stream);
}

template <class H>
int mg_cg_solve(void* handle, int sx, int sy, int sz, const int32_t* flags, float* dst, const float* rhs, float* residual, float* search,
                float* tmp, const float* A0, const float* Ai, const float* Aj, const float* Ak, float accuracy, int maxIter, int useL2Norm,
                float* out_host, void* stream) {
	Mg<H>* m = as_mg<H>(handle);
	if (!m) return fail("%s_cg_solve: bad handle", H::NAME);
	MF_TRY(check_dim(sx, sy, sz));
	const MgDim d0 = dim_of(m->v.l[0]);
	if (sx != d0.sx || sy != d0.sy || sz != d0.sz)
		return fail("%s_cg_solve: the hierarchy was created for %s, the system is %s", H::NAME, H::size_str(d0).s, H::size_str(MgDim{sx, sy, sz, 0}).s);
	const Dim d = mkdim(sx, sy, sz);
	PcExternal ext = {ext_init<H>, ext_apply<H>, m};
	return cg_solve_external(d, flags, dst, rhs, residual, search, tmp, A0, Ai, Aj, Ak, &ext, accuracy, maxIter, useL2Norm, out_host, stream);
}

template <class H>
int mg_info(void* handle, int64_t* out_host, int n_out) {
	Mg<H>* m = as_mg<H>(handle);
	if (!m) return fail("%s_info: bad handle", H::NAME);
	if (n_out < 8 + 4 * m->v.nl) return fail("%s_info: out_host holds %d entries, %d needed", H::NAME, n_out, 8 + 4 * m->v.nl);
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
		const MgDim d = dim_of(m->v.l[l]);
		out_host[8 + 4 * l] = d.sx;
		out_host[9 + 4 * l] = d.sy;
		out_host[10 + 4 * l] = d.sz;
		out_host[11 + 4 * l] = m->aset ? m->nactive[l] : 0;
	}
	return 0;
}

template <class H>
int mg_read_level(void* handle, int level, int what, void* dst_host, int64_t bytes) {
	Mg<H>* m = as_mg<H>(handle);
	if (!m) return fail("%s_read_level: bad handle", H::NAME);
	if (level < 0 || level >= m->v.nl) return fail("%s_read_level: level %d of %d", H::NAME, level, m->v.nl);
	const typename H::Lv& L = m->v.l[level];
	const void* src;
	int64_t want;
	switch (what) {
		case 0: src = L.t; want = L.n; break;
		case 1: src = L.A; want = (int64_t)L.n * H::planes(level == 0) * sizeof(float); break;
		case 2: src = L.x; want = (int64_t)L.n * sizeof(float); break;
		case 3: src = L.b; want = (int64_t)L.n * sizeof(float); break;
		default: return fail("%s_read_level: what = %d", H::NAME, what);
	}
	if (bytes != want) return fail("%s_read_level: %lld bytes given, the array has %lld", H::NAME, (long long)bytes, (long long)want);
	MF_HIP(hipDeviceSynchronize());
	MF_HIP(hipMemcpy(dst_host, src, (size_t)want, hipMemcpyDeviceToHost));
	return 0;
}

}  // namespace
}  // namespace mf
