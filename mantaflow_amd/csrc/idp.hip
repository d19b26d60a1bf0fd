// idp.hip -- implicit density projection (include/manta_hip_idp.h): the marking of fluid cells with the push-out displacements of
// particles inside obstacles, the density of the particle distribution (knComputeDensity as its single-thread sweep), the
// displacement field of the position solve and its gather to the particle positions.  Reference:
// source/plugin/implicitdensityprojection.cpp.  The order-free statements of its two serial loops are in DESIGN.md ("Implicit
// density projection").
#include "common.h"
#include "../../include/manta_hip_idp.h"

using namespace mf;

namespace {

Arena g_arena[MAX_DEVICES];   // this file's per-device scratch (arena_reserve): grows geometrically, never shrinks

// relaxed agent-scope accesses for words that one kernel writes and reads (the rounds of the density sweep)
__device__ __forceinline__ int ld_agent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- marking -------------------------------------------------------------------------------------------------------------------
// knClearFluidFlags, :29-33
__global__ __launch_bounds__(BLOCK) void k_clear_fluid(int64_t n, int32_t* __restrict__ flags) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	const int f = flags[idx];
	if (f & MF_FLUID) flags[idx] = (f | MF_EMPTY) & ~MF_FLUID;
}

// :41-47.  No cell carries the fluid bit after the clear, so "was empty when the loop began" is (empty | fluid) at any moment of
// this kernel: every particle of such a cell writes the same word.  A particle of an obstacle cell goes to the list.
__global__ __launch_bounds__(BLOCK) void k_mark(Dim d, int32_t* __restrict__ flags, int64_t np, int64_t ps, const float* __restrict__ pos,
                                                const int32_t* __restrict__ pflag, const int32_t* __restrict__ ptype, int exclude,
                                                int32_t* __restrict__ list, unsigned long long* __restrict__ cnt) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= np) return;
	if ((pflag[p] & MF_PDELETE) || (ptype && (ptype[p] & exclude))) return;
	const int i = (int)pos[p], j = (int)pos[ps + p], k = (int)pos[2 * ps + p];   // toVec3i: truncation
	if (i < 0 || j < 0 || k < 0 || i >= d.sx || j >= d.sy || k >= d.sz) return;
	const int64_t idx = (int64_t)i + d.Y * j + d.Z * k;
	const int f = flags[idx];
	if (f & (MF_EMPTY | MF_FLUID)) {
		if (f & MF_EMPTY) flags[idx] = (f | MF_FLUID) & ~MF_EMPTY;
	} else if (f & MF_OBSTACLE) {
		list[atomicAdd(cnt, 1ull)] = (int32_t)p;
	}
}

// :49-60: the proposal of one particle inside an obstacle cell; false when phiObs > 0 there
__device__ __forceinline__ bool push_out(const Dim& d, const float* __restrict__ phi, float x, float y, float z, float dir[3]) {
	float dist = interpol1(d, phi, x, y, z);
	if (dist > 0.f) return false;
	const float eps = 1.0e-3f, e2 = 2.0f * eps;
	dir[0] = (interpol1(d, phi, x + eps, y, z) - interpol1(d, phi, x - eps, y, z)) / e2;
	dir[1] = (interpol1(d, phi, x, y + eps, z) - interpol1(d, phi, x, y - eps, z)) / e2;
	dir[2] = 0.f;
	if (d.is3d) dir[2] = (interpol1(d, phi, x, y, z + eps) - interpol1(d, phi, x, y, z - eps)) / e2;
	if (dist < -1.0f) dist = -1.0f;
	const double s = -((double)dist + 1.0e-2);
#pragma unroll
	for (int c = 0; c < 3; c++) dir[c] = (float)(s * (double)dir[c]);
	return true;
}

// The four passes over the list.  A face keeps the proposal with the largest |value|, ties to the lowest particle index (:65-75):
//   PASS 0  deltaX(face) = max |value| (the bit pattern of a non-negative float orders like an unsigned integer)
//   PASS 1  owner(face) = INT_MAX on every face some proposal reaches the maximum of
//   PASS 2  owner(face) = min particle index among those proposals
//   PASS 3  the owner writes its signed value
// Proposals of magnitude 0 and NaN never pass the reference's `>` and take no part.
template <int PASS>
__global__ __launch_bounds__(BLOCK) void k_push(Dim d, const float* __restrict__ phi, int64_t nb, const int32_t* __restrict__ list,
                                                int64_t ps, const float* __restrict__ pos, float* __restrict__ deltaX,
                                                int32_t* __restrict__ owner, unsigned long long* __restrict__ cnt) {
	const int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (q >= nb) return;
	const int p = list[q];
	const float x = pos[p], y = pos[ps + p], z = pos[2 * ps + p];
	float dir[3];
	if (!push_out(d, phi, x, y, z, dir)) return;
	if (PASS == 0) atomicAdd(cnt + 1, 1ull);
	const int c3[3] = {(int)x, (int)y, (int)z};
	const int sz3[3] = {d.sx, d.sy, d.sz};
	const int64_t st3[3] = {1, d.Y, d.Z};
	const int64_t idx = (int64_t)c3[0] + d.Y * c3[1] + d.Z * c3[2];
	const int nc = d.is3d ? 3 : 2;
	for (int c = 0; c < nc; c++) {
		const unsigned bits = __float_as_uint(dir[c]) & 0x7fffffffu;
		if (bits == 0u || bits > 0x7f800000u) continue;
		for (int e = 0; e < 2; e++) {
			if (e && c3[c] + 1 >= sz3[c]) continue;
			const int64_t face = (int64_t)c * d.n + idx + (e ? st3[c] : 0);
			if (PASS == 0) {
				atomicMax((unsigned*)deltaX + face, bits);
			} else {
				if ((__float_as_uint(deltaX[face]) & 0x7fffffffu) != bits) continue;
				if (PASS == 1) owner[face] = 0x7fffffff;
				if (PASS == 2) atomicMin(owner + face, p);
				if (PASS == 3 && owner[face] == p) deltaX[face] = dir[c];
			}
		}
	}
}

// ---- density -------------------------------------------------------------------------------------------------------------------
// a flag / a MAC component at a cell that may lie outside the grid (fluid on the outermost layer is outside the contract; it must
// not fault): nothing there
__device__ __forceinline__ int flag_at(const Dim& d, const int32_t* __restrict__ f, int i, int j, int k) {
	return in_grid(d, i, j, k) ? f[(int64_t)i + d.Y * j + d.Z * k] : 0;
}
__device__ __forceinline__ float mac_at(const Dim& d, const float* __restrict__ g, int i, int j, int k) {
	return in_grid(d, i, j, k) ? g[(int64_t)i + d.Y * j + d.Z * k] : 0.f;
}
// :106-110: 1 - w * mass minus the divergence of the push-out displacements
__device__ __forceinline__ float density_base(const Dim& d, float w, float mass, const float* __restrict__ dX, int64_t idx, int i, int j, int k) {
	float dens = 1.0f - w * mass;
	dens -= dX[idx] - mac_at(d, dX, i + 1, j, k) + dX[d.n + idx] - mac_at(d, dX + d.n, i, j + 1, k);
	if (d.is3d) dens -= dX[2 * d.n + idx] - mac_at(d, dX + 2 * d.n, i, j, k + 1);
	return dens;
}
// :113-114 on the entry flags
__device__ __forceinline__ bool is_surface(const Dim& d, const int32_t* __restrict__ f0, int i, int j, int k) {
	bool s = (flag_at(d, f0, i - 1, j, k) & MF_EMPTY) || (flag_at(d, f0, i + 1, j, k) & MF_EMPTY) || (flag_at(d, f0, i, j - 1, k) & MF_EMPTY) ||
	         (flag_at(d, f0, i, j + 1, k) & MF_EMPTY);
	if (d.is3d) s = s || (flag_at(d, f0, i, j, k - 1) & MF_EMPTY) || (flag_at(d, f0, i, j, k + 1) & MF_EMPTY);
	return s;
}
// :121-132, the particle-deficiency loop in its l, m, n order; nf(l, m, n) is the flag the sweep sees at (i + l, j + m, k + n).  The
// branch conditions are the reference's, with the cell's own k where the loop variable n is meant.
template <class NF>
__device__ __forceinline__ float deficiency(float dens, int k, float mass, NF nf) {
	const float N[3] = {0.25f, 0.75f, 0.25f};
	for (int l = -1; l < 2; l++)
		for (int m = -1; m < 2; m++)
			for (int n = -1; n < 2; n++)
				if (nf(l, m, n) & (MF_OBSTACLE | MF_EMPTY)) {
					const float w = N[l + 1] * N[m + 1] * N[n + 1] * mass;
					if ((l == 0 && m == 0) || (l == 0 && k == 0) || (m == 0 && k == 0))
						dens = (float)((double)dens - (double)w * 4.0);
					else if ((l != 0 && m != 0) || (l != 0 && k != 0) || (m != 0 && k != 0))
						dens = (float)((double)dens - (double)w * 2.0);
					else
						dens = dens - w;
				}
	return dens;
}
__device__ __forceinline__ bool swept_before(int l, int m, int n) { return n < 0 || (n == 0 && (m < 0 || (m == 0 && l < 0))); }

// 3-D, first pass: the cells whose flip depends on the flips of cells swept before them.  More empty neighbours only lower a cell's
// density (mass >= 0: every step of the chain is monotone), so a surface cell that is not positive against the entry flags never
// flips; with a negative mass every surface cell is a candidate.
__global__ __launch_bounds__(BLOCK) void k_density_candidates(Dim d, const float* __restrict__ dens, const int32_t* __restrict__ f0,
                                                              const float* __restrict__ dX, float mass, int32_t* __restrict__ state,
                                                              int32_t* __restrict__ cand, unsigned long long* __restrict__ cnt) {
	CELL_IJK(d)
	int st = 0;
	if ((f0[idx] & MF_FLUID) && is_surface(d, f0, i, j, k)) {
		const float v = deficiency(density_base(d, dens[idx], mass, dX, idx, i, j, k), k, mass,
		                           [&](int l, int m, int n) { return flag_at(d, f0, i + l, j + m, k + n); });
		if (mass < 0.f || v > 0.f) {
			st = 1;
			cand[atomicAdd(cnt, 1ull)] = (int32_t)idx;
		}
	}
	state[idx] = st;
}

// 3-D, the rounds, one workgroup: a candidate is decided in the first round in which none of the 13 cells swept before it is an
// undecided candidate; it then sees their final flags in `flags` and the entry flags of the cells after it (a candidate after it
// waits for it, a cell that is no candidate never flips).  Decisions of a round are applied after the round's barrier.
constexpr int RBLOCK = 1024;
__global__ __launch_bounds__(RBLOCK) void k_density_rounds(Dim d, const float* __restrict__ dens, int32_t* flags, const float* __restrict__ dX,
                                                           float mass, int32_t* state, int32_t* cand, unsigned long long* cnt) {
	const int64_t nc = (int64_t)cnt[0];
	unsigned long long rounds = 0;
	for (;;) {
		int left = 0;
		for (int64_t q = threadIdx.x; q < nc; q += RBLOCK) {
			const int c = cand[q];
			if (c < 0) continue;   // decided in an earlier round
			const unsigned t_ = (unsigned)c / (unsigned)d.sx;
			const int i = (int)((unsigned)c - t_ * (unsigned)d.sx), j = (int)(t_ % (unsigned)d.sy), k = (int)(t_ / (unsigned)d.sy);
			bool wait = false;
			for (int n = -1; n < 1 && !wait; n++)
				for (int m = -1; m < 2 && !wait; m++)
					for (int l = -1; l < 2; l++)
						if (swept_before(l, m, n) && in_grid(d, i + l, j + m, k + n) &&
						    ld_agent(state + ((int64_t)(i + l) + d.Y * (j + m) + d.Z * (k + n))) == 1) {
							wait = true;
							break;
						}
			if (wait) {
				left = 1;
				continue;
			}
			const float v = deficiency(density_base(d, dens[c], mass, dX, c, i, j, k), k, mass, [&](int l, int m, int n) {
				return in_grid(d, i + l, j + m, k + n) ? ld_agent(flags + ((int64_t)(i + l) + d.Y * (j + m) + d.Z * (k + n))) : 0;
			});
			cand[q] = v > 0.f ? -2 : -3;   // this thread's slot: read by it alone
			left = 1;                      // to be applied below
		}
		__threadfence_block();
		if (!__syncthreads_or(left)) break;
		rounds++;
		for (int64_t q = threadIdx.x; q < nc; q += RBLOCK) {
			const int c = cand[q];
			if (c == -2 || c == -3) {
				// the cell index went with the decision: keep it beside the list
				const int cell = cand[nc + q];
				if (c == -2) st_agent(flags + cell, MF_EMPTY);
				st_agent(state + cell, 2);
				cand[q] = -1;
			}
		}
		__threadfence_block();
		__syncthreads();
	}
	if (threadIdx.x == 0) cnt[2] = rounds;
}
__global__ __launch_bounds__(BLOCK) void k_copy_cand(int32_t* cand, const unsigned long long* cnt) {
	const int64_t nc = (int64_t)cnt[0];
	for (int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x; q < nc; q += (int64_t)gridDim.x * BLOCK) cand[nc + q] = cand[q];
}

// :104-153 for every cell, with the flags as the sweep sees them: `flags` (final) at the cells before this one, f0 at itself and after
// it.  In 3-D the flips are in `flags` already (k_density_rounds; the condition below is true for exactly those cells); in 2-D the
// kernel is a plain map and writes them.
__global__ __launch_bounds__(BLOCK) void k_density_final(Dim d, float* __restrict__ dens, const int32_t* __restrict__ f0, int32_t* flags,
                                                         const float* __restrict__ dX, float dt, float mass, int noClamp,
                                                         unsigned long long* __restrict__ cnt) {
	CELL_IJK(d)
	if (!(f0[idx] & MF_FLUID)) {
		dens[idx] = 0.f;
		return;
	}
	float v = density_base(d, dens[idx], mass, dX, idx, i, j, k);
	if (d.is3d)
		v = deficiency(v, k, mass, [&](int l, int m, int n) { return flag_at(d, swept_before(l, m, n) ? flags : f0, i + l, j + m, k + n); });
	if (is_surface(d, f0, i, j, k) && v > 0.f) {
		if (!d.is3d) flags[idx] = MF_EMPTY;
		v = 0.f;
		atomicAdd(cnt + 1, 1ull);
	}
	if (!noClamp) {
		if (v < -0.5f) v = -0.5f;
		if (v > 0.5f) v = 0.5f;
		v = v / dt;
	}
	dens[idx] = v;
}

// ---- displacements ----------------------------------------------------------------------------------------------------------------
// knRemoveEmptyLambdas + knComputeDeltaX, :184-199, in one pass: the Lambda a neighbour ends with depends on its flag alone
__global__ __launch_bounds__(BLOCK) void k_compute_delta_x(Dim d, const int32_t* __restrict__ flags, float* __restrict__ dX, float* Lambda) {
	CELL_IJK(d)
	auto lam = [&](int ii, int jj, int kk) {
		const int64_t c = (int64_t)ii + d.Y * jj + d.Z * kk;
		const bool inner = ii >= 1 && ii <= d.sx - 2 && jj >= 1 && jj <= d.sy - 2 && (!d.is3d || (kk >= 1 && kk <= d.sz - 2));
		return (inner && (flags[c] & MF_EMPTY)) ? 0.f : Lambda[c];
	};
	const float here = lam(i, j, k);
	const int f = flags[idx];
	if (!(f & MF_OBSTACLE)) {
		if (i > 0 && !(flags[idx - 1] & MF_OBSTACLE)) dX[idx] = here - lam(i - 1, j, k);
		if (j > 0 && !(flags[idx - d.Y] & MF_OBSTACLE)) dX[d.n + idx] = here - lam(i, j - 1, k);
		if (d.is3d && k > 0 && !(flags[idx - d.Z] & MF_OBSTACLE)) dX[2 * d.n + idx] = here - lam(i, j, k - 1);
	}
	const bool inner = i >= 1 && i <= d.sx - 2 && j >= 1 && j <= d.sy - 2 && (!d.is3d || (k >= 1 && k <= d.sz - 2));
	if (inner && (f & MF_EMPTY)) Lambda[idx] = 0.f;
}

// knMapLinearMACGridToVec3_Position, :219-228, with clamp(), :207-215
__global__ __launch_bounds__(BLOCK) void k_map_positions(Dim d, const float* __restrict__ dX, int64_t np, int64_t ps, float* __restrict__ pos,
                                                         const int32_t* __restrict__ pflag, const int32_t* __restrict__ ptype, int exclude,
                                                         float dt) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= np) return;
	if ((pflag[p] & MF_PDELETE) || (ptype && (ptype[p] & exclude))) return;
	float x = pos[p], y = pos[ps + p], z = pos[2 * ps + p];
	float vx, vy, vz;
	// a 2-D grid has one plane: the sampler's z corners are that plane for z in [0, 1.5) (the scenes keep 0.5); outside it the plane
	// index would leave the grid, and the sample is taken at 0.5
	interpol_mac(d, dX, x, y, (d.is3d || (z >= 0.f && z < 1.5f)) ? z : 0.5f, vx, vy, vz);
	x += vx * dt;
	y += vy * dt;
	z += vz * dt;
	const float lo = 1.001f, hx = (float)d.sx - 1.001f, hy = (float)d.sy - 1.001f;
	const float lz = d.is3d ? 1.001f : -10.001f, hz = d.is3d ? (float)d.sz - 1.001f : 10.001f;
	if (x > hx) x = hx;
	if (x < lo) x = lo;
	if (y > hy) y = hy;
	if (y < lo) y = lo;
	if (z > hz) z = hz;
	if (z < lz) z = lz;
	pos[p] = x;
	pos[ps + p] = y;
	pos[2 * ps + p] = z;
}

}  // namespace

extern "C" {

int mf_idp_abi_version(void) { return MF_IDP_ABI_VERSION; }

int mf_idp_mark(int sx, int sy, int sz, int32_t* flags, float* deltaX, const float* phiObs, int64_t np, int64_t pstride,
                const float* pos, const int32_t* pflag, const int32_t* ptype, int exclude, int64_t* result_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	if (np < 0 || pstride < np || np >= ((int64_t)1 << 31)) return fail("markFluidAndBoundaryCells: bad particle range (np %lld, stride %lld)", (long long)np, (long long)pstride);
	const size_t nl = np > 0 ? np : 1, need = 256 + al256(sizeof(int32_t) * nl) + al256(sizeof(int32_t) * 3 * (size_t)d.n);
	Arena* a;
	MF_TRY(arena_reserve(g_arena, need, &a));
	Cutter c(a->p, need);
	unsigned long long* cnt;
	int32_t *list, *owner;
	MF_TRY(c.take(32, &cnt));
	MF_TRY(c.take(nl, &list));
	MF_TRY(c.take(3 * (size_t)d.n, &owner));
	MF_HIP(hipMemsetAsync(cnt, 0, 4 * sizeof(unsigned long long), st));
	MF_HIP(hipMemsetAsync(deltaX, 0, sizeof(float) * 3 * d.n, st));
	hipLaunchKernelGGL(k_clear_fluid, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d.n, flags);
	if (np > 0) hipLaunchKernelGGL(k_mark, dim3(nblk(np)), dim3(BLOCK), 0, st, d, flags, np, pstride, pos, pflag, ptype, exclude, list, cnt);
	MF_LAUNCH_CHECK();
	MF_TRY(read_back(result_host, cnt, sizeof(int64_t), st));
	const int64_t nb = result_host[0];
	result_host[1] = 0;
	if (nb > 0) {
		const dim3 g(nblk(nb)), b(BLOCK);
		hipLaunchKernelGGL((k_push<0>), g, b, 0, st, d, phiObs, nb, list, pstride, pos, deltaX, owner, cnt);
		hipLaunchKernelGGL((k_push<1>), g, b, 0, st, d, phiObs, nb, list, pstride, pos, deltaX, owner, cnt);
		hipLaunchKernelGGL((k_push<2>), g, b, 0, st, d, phiObs, nb, list, pstride, pos, deltaX, owner, cnt);
		hipLaunchKernelGGL((k_push<3>), g, b, 0, st, d, phiObs, nb, list, pstride, pos, deltaX, owner, cnt);
		MF_LAUNCH_CHECK();
		MF_TRY(read_back(result_host + 1, cnt + 1, sizeof(int64_t), st));
	}
	return 0;
}

int mf_idp_map_weights(int sx, int sy, int sz, float* density, int64_t np, int64_t pstride, const float* pos, const int32_t* pflag,
                       const float* psrc, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	MF_HIP(hipMemsetAsync(density, 0, sizeof(float) * d.n, st));
	if (np <= 0) return 0;
	// the value grid of the transfer (knMapLinear's `tmp` role swapped: it receives the weighted sources) is discarded
	const size_t need = al256(sizeof(float) * (size_t)d.n);
	Arena* a;
	MF_TRY(arena_reserve(g_arena, need, &a));
	float* values;
	MF_TRY(Cutter(a->p, need).take(d.n, &values));
	return p2g_ordered_cell(d, 1, values, density, np, pstride, pos, pflag, psrc, st);
}

int mf_idp_compute_density(int sx, int sy, int sz, float* density, int32_t* flags, const float* deltaX, float dt, float mass,
                           int noDensityClamping, int64_t* result_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	const size_t need = 256 + 4 * al256(sizeof(int32_t) * (size_t)d.n);
	Arena* a;
	MF_TRY(arena_reserve(g_arena, need, &a));
	Cutter c(a->p, need);
	unsigned long long* cnt;
	int32_t *f0, *state, *cand;
	MF_TRY(c.take(32, &cnt));
	MF_TRY(c.take(d.n, &f0, &state));
	MF_TRY(c.take(2 * (size_t)d.n, &cand));   // 2 n words: the list, and its copy that keeps the cell of a decided slot
	MF_HIP(hipMemsetAsync(cnt, 0, 4 * sizeof(unsigned long long), st));
	MF_HIP(hipMemcpyAsync(f0, flags, sizeof(int32_t) * d.n, hipMemcpyDeviceToDevice, st));   // FlagGrid flagsTmp(flags), :162
	const dim3 g(nblk(d.n)), b(BLOCK);
	if (d.is3d) {
		hipLaunchKernelGGL(k_density_candidates, g, b, 0, st, d, density, f0, deltaX, mass, state, cand, cnt);
		hipLaunchKernelGGL(k_copy_cand, dim3(256), b, 0, st, cand, cnt);
		hipLaunchKernelGGL(k_density_rounds, dim3(1), dim3(RBLOCK), 0, st, d, density, flags, deltaX, mass, state, cand, cnt);
	}
	hipLaunchKernelGGL(k_density_final, g, b, 0, st, d, density, f0, flags, deltaX, dt, mass, noDensityClamping, cnt);
	MF_LAUNCH_CHECK();
	return read_back(result_host, cnt, 4 * sizeof(int64_t), st);
}

int mf_idp_compute_delta_x(int sx, int sy, int sz, const int32_t* flags, float* deltaX, float* Lambda, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_compute_delta_x, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, deltaX, Lambda);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_idp_map_mac_to_positions(int sx, int sy, int sz, const float* deltaX, int64_t np, int64_t pstride, float* pos,
                                const int32_t* pflag, const int32_t* ptype, int exclude, float dt, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	if (np <= 0) return 0;
	if (pstride < np) return fail("mapMACToPartPositions: particle stride %lld below %lld", (long long)pstride, (long long)np);
	hipLaunchKernelGGL(k_map_positions, dim3(nblk(np)), dim3(BLOCK), 0, (hipStream_t)stream, d, deltaX, np, pstride, pos, pflag, ptype,
	                   exclude, dt);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
