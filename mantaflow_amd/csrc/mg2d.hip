// mg2d.hip -- the multigrid preconditioner of the pressure PCG on 2-D grids, gfx950 (include/open/manta_hip_mg2d.h).
// Reference: source/multigrid.{h,cpp} (GridMg with mIs3D == false, cited per function in mg2d_cells.h),
// source/conjugategrad.cpp:100-106, 162-167 (PC_MGP).  The 3-D hierarchy is multigrid.hip; the two share the host side of the
// set-up (mg_host.h) and nothing of their device code.
//
// Every pass of a V-cycle (a colour of the smoother, the residual, restriction, interpolation) is a function of mg2d_cells.h
// over "work items start, start + stride, ..." and is used twice: by a grid-wide kernel (one item per thread) on the large
// levels, and by the single-workgroup tail kernel k_mg2d_tail, which runs every level of at most TAIL_VERTS vertices -- down,
// the coarsest-level CG, and up again -- in ONE launch with workgroup barriers between the passes.  A 2-D pyramid is deeper
// than a 3-D one of the same cell count (a level has a quarter of the vertices of the one below it, not an eighth), and
// every level below some ten thousand vertices is launch-bound: the tail takes 9 launches per level away.
//
// Set-up: the greedy coarse-vertex selection (genCoarseGrid) is serial and order-dependent; it runs on the host on the
// downloaded type bytes, with the reference's bucket heap order.  Everything else of the set-up is a gather per vertex on the
// device.
#include "mg2d_cells.h"
#include "pressure.h"
#include "../../include/open/manta_hip_mg2d.h"
#include <chrono>
#include <stdlib.h>

using namespace mf;
using namespace mf::mg2d;

namespace {

constexpr int TAIL_BLOCK = 1024;      // one workgroup; the coarsest level has at most 1000 vertices (one per thread in the CG)
constexpr int TAIL_VERTS = 8192;      // levels of at most this many vertices run inside k_mg2d_tail
constexpr unsigned MG2D_MAGIC = 0x4d473244u;

struct Mg2 {
	unsigned magic;
	int dev;
	View v;
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

// ---------------------------------------------------------------------------------------------------------
// grid-wide forms: one item per thread
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
k_mg2d_copy_activate(Lv L, const float* __restrict__ A0, const float* __restrict__ Ai, const float* __restrict__ Aj, int* __restrict__ info) {
	const int v = blockIdx.x * BLOCK + threadIdx.x;
	if (v < L.n) copy_activate(L, v, A0, Ai, Aj, info);
}
__global__ void __launch_bounds__(BLOCK) k_mg2d_operator1(Lv F, Lv C, const Path* __restrict__ paths, int npaths) {
	const int idx = blockIdx.x * BLOCK + threadIdx.x;
	if (idx < C.n) operator1(F, C, idx, paths, npaths);
}
__global__ void __launch_bounds__(BLOCK) k_mg2d_operatorN(Lv F, Lv C) {
	const int idx = blockIdx.x * BLOCK + threadIdx.x;
	if (idx < C.n) operatorN(F, C, idx);
}
__global__ void __launch_bounds__(BLOCK) k_mg2d_smooth(Lv L, int l0, int colour) {
	pass_smooth(L, l0 != 0, colour, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK);
}
__global__ void __launch_bounds__(BLOCK) k_mg2d_residual(Lv L, int l0) { pass_residual(L, l0 != 0, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK); }
__global__ void __launch_bounds__(BLOCK) k_mg2d_restrict(Lv F, Lv C) { pass_restrict(F, C, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK); }
__global__ void __launch_bounds__(BLOCK) k_mg2d_interp_add(Lv F, Lv C) { pass_interp_add(F, C, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK); }
__global__ void __launch_bounds__(BLOCK) k_mg2d_set_rhs(Lv L, const float* __restrict__ rhs) {
	const int v = blockIdx.x * BLOCK + threadIdx.x;
	if (v < L.n) set_rhs(L, v, rhs);
}

// ---------------------------------------------------------------------------------------------------------
// the tail: every level from `first` down, solveCG on the coarsest, and up again, in one workgroup
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TAIL_BLOCK)
k_mg2d_tail(View M, int first, float accuracy, int* __restrict__ info) {
	__shared__ double s_vec[TAIL_BLOCK];
	__shared__ double s_r1[TAIL_BLOCK];
	__shared__ double s_r2[TAIL_BLOCK];
	__shared__ double s_out[2];
	const int tid = threadIdx.x;
	const int last = M.nl - 1;
	// down, multigrid.cpp:460-475
	for (int l = first; l < last; l++) {
		const Lv& L = M.l[l];
		for (int c = 0; c < smooth_colours(l == 0); c++) {
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
		const int X = in ? v % L.sx : 0, Y = in ? v / L.sx : 0;
		const float diag = act ? L.A[v] : 1.f;
		double x = in ? (double)L.x[v] : 0.0, r = 0.0, z = 0.0, p = 0.0;
		s_vec[tid] = x;
		__syncthreads();
		if (act) {
			r = L.b[v] - cg_apply(L, l0, v, X, Y, s_vec);
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
			if (act) z = cg_apply(L, l0, v, X, Y, s_vec);
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
		for (int c = smooth_colours(l == 0) - 1; c >= 0; c--) {
			pass_smooth(L, l == 0, c, tid, TAIL_BLOCK);
			__syncthreads();
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
// the handles that mf_mg2d_create gave out and mf_mg2d_destroy has not taken back (mg_host.h)
LiveHandles g_live;
Mg2* as_mg(void* h) {
	if (!h || !g_live.has(h)) return nullptr;
	Mg2* m = (Mg2*)h;
	return m->magic == MG2D_MAGIC ? m : nullptr;
}

void free_levels(Mg2* m) {
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

int mg_set_a(Mg2* m, const float* A0, const float* Ai, const float* Aj, hipStream_t st) {
	using clk = std::chrono::steady_clock;
	const auto t0 = clk::now();
	int64_t us_host = 0;
	View& V = m->v;
	MF_HIP(hipMemsetAsync(m->d_info, 0, 3 * sizeof(int), st));
	hipLaunchKernelGGL(k_mg2d_copy_activate, dim3(nblk(V.l[0].n)), dim3(BLOCK), 0, st, V.l[0], A0, Ai, Aj, m->d_info);
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
		if (l == 1) hipLaunchKernelGGL(k_mg2d_operator1, dim3(nblk(V.l[l].n)), dim3(BLOCK), 0, st, V.l[0], V.l[1], m->paths, m->npaths);
		else hipLaunchKernelGGL(k_mg2d_operatorN, dim3(nblk(V.l[l].n)), dim3(BLOCK), 0, st, V.l[l - 1], V.l[l]);
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

int mg_vcycle(Mg2* m, float* dst, const float* rhs, hipStream_t st) {
	if (!m->aset) return fail("mf_mg2d_vcycle: GridMg::setRhs Error: A has not been set.");
	const View& V = m->v;
	const int first = m->tail_first;
	hipLaunchKernelGGL(k_mg2d_set_rhs, dim3(nblk(V.l[0].n)), dim3(BLOCK), 0, st, V.l[0], rhs);
	for (int l = 0; l < first; l++) {
		const Lv& L = V.l[l];
		const int l0 = l == 0;
		const int items = smooth_items(L, l0);
		for (int c = 0; c < smooth_colours(l0); c++) hipLaunchKernelGGL(k_mg2d_smooth, dim3(nblk(items)), dim3(BLOCK), 0, st, L, l0, c);
		hipLaunchKernelGGL(k_mg2d_residual, dim3(nblk(L.n)), dim3(BLOCK), 0, st, L, l0);
		hipLaunchKernelGGL(k_mg2d_restrict, dim3(nblk(V.l[l + 1].n)), dim3(BLOCK), 0, st, L, V.l[l + 1]);
	}
	hipLaunchKernelGGL(k_mg2d_tail, dim3(1), dim3(TAIL_BLOCK), 0, st, V, first, m->coarsestAcc, m->d_info);
	for (int l = first - 1; l >= 0; l--) {
		const Lv& L = V.l[l];
		const int l0 = l == 0;
		const int items = smooth_items(L, l0);
		hipLaunchKernelGGL(k_mg2d_interp_add, dim3(nblk(L.n)), dim3(BLOCK), 0, st, L, V.l[l + 1]);
		for (int c = smooth_colours(l0) - 1; c >= 0; c--) hipLaunchKernelGGL(k_mg2d_smooth, dim3(nblk(items)), dim3(BLOCK), 0, st, L, l0, c);
	}
	MF_LAUNCH_CHECK();
	MF_HIP(hipMemcpyAsync(dst, V.l[0].x, sizeof(float) * V.l[0].n, hipMemcpyDeviceToDevice, st));      // knCopyToGrid, multigrid.cpp:499
	return 0;
}

// PcExternal hands four planes over; a 2-D system has no Ak and the hierarchy does not look at it
int ext_init(void* ctx, const float* A0, const float* Ai, const float* Aj, const float*, float accuracy, hipStream_t st) {
	Mg2* m = (Mg2*)ctx;
	if (!m->aset) MF_TRY(mg_set_a(m, A0, Ai, Aj, st));      // InitPreconditionMultigrid, conjugategrad.cpp:100-106
	m->coarsestAcc = (float)(accuracy * 1E-4);
	return 0;
}
int ext_apply(void* ctx, float* dst, const float* src, hipStream_t st) { return mg_vcycle((Mg2*)ctx, dst, src, st); }

}  // namespace

extern "C" {

int mf_mg2d_abi_version(void) { return MF_MG2D_ABI_VERSION; }

int mf_mg2d_create(int sx, int sy, void** handle_out) {
	if (!handle_out) return fail("mf_mg2d_create: null handle_out");
	*handle_out = nullptr;
	MF_TRY(check_dim(sx, sy, 1));
	Mg2* m = new Mg2();
	m->magic = MG2D_MAGIC;
	m->coarsestAcc = 1E-8f;
	MF_HIP(hipGetDevice(&m->dev));
	View& V = m->v;
	int sizes[MAXL][2];
	const int nl = pyramid(sx, sy, sizes);
	int rc = 0;
	for (int l = 0; l < nl; l++) {
		Lv& L = V.l[l];
		L.sx = sizes[l][0];
		L.sy = sizes[l][1];
		L.n = L.sx * L.sy;
		const size_t na = (size_t)L.n * (l == 0 ? 3 : 5) * sizeof(float), nv = (size_t)L.n * sizeof(float);
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
			rc = fail("mf_mg2d_create: level %d (%d x %d): %s", l, L.sx, L.sy, hipGetErrorString(e));
			break;
		}
	}
	// (the pyramid rule leaves at most 1000 vertices on the last level unless MAXL levels did not reach it)
	if (rc == 0 && V.l[V.nl - 1].n > TAIL_BLOCK) rc = fail("mf_mg2d_create: coarsest level has %d vertices (at most %d supported)", V.l[V.nl - 1].n, TAIL_BLOCK);
	if (rc == 0) {
		const std::vector<Path> ps = make_paths();
		m->npaths = (int)ps.size();
		hipError_t e = hipMalloc((void**)&m->paths, ps.size() * sizeof(Path));
		if (e == hipSuccess) e = hipMemcpy(m->paths, ps.data(), ps.size() * sizeof(Path), hipMemcpyHostToDevice);
		if (e == hipSuccess) e = hipMalloc((void**)&m->d_info, 4 * sizeof(int));
		if (e == hipSuccess) e = hipMemset(m->d_info, 0, 4 * sizeof(int));
		if (e != hipSuccess) rc = fail("mf_mg2d_create: %s", hipGetErrorString(e));
	}
	if (rc != 0) {
		(void)hipGetLastError();
		free_levels(m);
		m->magic = 0;
		delete m;
		return rc;
	}
	// the single-workgroup tail takes every level of at most TAIL_VERTS vertices, and always the coarsest (MF_MG_TAIL_VERTS: the
	// measurement knob of the 3-D hierarchy -- 0 leaves the tail the coarsest-level CG alone; the results do not depend on it)
	int tail_verts = TAIL_VERTS;
	if (const char* e = getenv("MF_MG_TAIL_VERTS")) tail_verts = atoi(e);
	m->tail_first = V.nl - 1;
	while (m->tail_first > 0 && V.l[m->tail_first - 1].n <= tail_verts) m->tail_first--;
	g_live.insert(m);
	*handle_out = m;
	return 0;
}

int mf_mg2d_destroy(void* handle) {
	Mg2* m = as_mg(handle);
	if (!m) return fail("mf_mg2d_destroy: bad handle");
	MF_HIP(hipDeviceSynchronize());
	g_live.erase(handle);
	free_levels(m);
	m->magic = 0;
	delete m;
	return 0;
}

int mf_mg2d_set_a(void* handle, const float* A0, const float* Ai, const float* Aj, void* stream) {
	Mg2* m = as_mg(handle);
	if (!m) return fail("mf_mg2d_set_a: bad handle");
	return mg_set_a(m, A0, Ai, Aj, (hipStream_t)stream);
}

int mf_mg2d_is_a_set(void* handle) {
	Mg2* m = as_mg(handle);
	return m ? (m->aset ? 1 : 0) : -1;
}

int mf_mg2d_vcycle(void* handle, float* dst, const float* rhs, void* stream) {
	Mg2* m = as_mg(handle);
	if (!m) return fail("mf_mg2d_vcycle: bad handle");
	return mg_vcycle(m, dst, rhs, (hipStream_t)stream);
}

int mf_mg2d_cg_solve(void* handle, int sx, int sy, const int32_t* flags, float* dst, const float* rhs, float* residual,
                     float* search, float* tmp, const float* A0, const float* Ai, const float* Aj, float accuracy,
                     int maxIter, int useL2Norm, float* out_host, void* stream) {
	Mg2* m = as_mg(handle);
	if (!m) return fail("mf_mg2d_cg_solve: bad handle");
	MF_TRY(check_dim(sx, sy, 1));
	const Lv& L0 = m->v.l[0];
	if (sx != L0.sx || sy != L0.sy)
		return fail("mf_mg2d_cg_solve: the hierarchy was created for %d x %d, the system is %d x %d", L0.sx, L0.sy, sx, sy);
	const Dim d = mkdim(sx, sy, 1);
	PcExternal ext = {ext_init, ext_apply, m};
	return cg_solve_external(d, flags, dst, rhs, residual, search, tmp, A0, Ai, Aj, nullptr, &ext, accuracy, maxIter, useL2Norm, out_host, stream);
}

int mf_mg2d_info(void* handle, int64_t* out_host, int n_out) {
	Mg2* m = as_mg(handle);
	if (!m) return fail("mf_mg2d_info: bad handle");
	if (n_out < 8 + 4 * m->v.nl) return fail("mf_mg2d_info: out_host holds %d entries, %d needed", n_out, 8 + 4 * m->v.nl);
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
		out_host[10 + 4 * l] = 1;
		out_host[11 + 4 * l] = m->aset ? m->nactive[l] : 0;
	}
	return 0;
}

int mf_mg2d_read_level(void* handle, int level, int what, void* dst_host, int64_t bytes) {
	Mg2* m = as_mg(handle);
	if (!m) return fail("mf_mg2d_read_level: bad handle");
	if (level < 0 || level >= m->v.nl) return fail("mf_mg2d_read_level: level %d of %d", level, m->v.nl);
	const Lv& L = m->v.l[level];
	const void* src;
	int64_t want;
	switch (what) {
		case 0: src = L.t; want = L.n; break;
		case 1: src = L.A; want = (int64_t)L.n * (level == 0 ? 3 : 5) * sizeof(float); break;
		case 2: src = L.x; want = (int64_t)L.n * sizeof(float); break;
		case 3: src = L.b; want = (int64_t)L.n * sizeof(float); break;
		default: return fail("mf_mg2d_read_level: what = %d", what);
	}
	if (bytes != want) return fail("mf_mg2d_read_level: %lld bytes given, the array has %lld", (long long)bytes, (long long)want);
	MF_HIP(hipDeviceSynchronize());
	MF_HIP(hipMemcpy(dst_host, src, (size_t)want, hipMemcpyDeviceToHost));
	return 0;
}

}  // extern "C"
