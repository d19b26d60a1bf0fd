// resample.hip -- particle resampling for narrow-band FLIP (include/manta_hip_resample.h): adjustNumber's particle loop in its
// order-free form, the particle system's compress, the seeding loop with the buffered insertion, combineGridVel, and the grid
// operations setBoundNeumann / initFromFlags.  Reference: source/plugin/flip.cpp, source/particle.{h,cpp}, source/grid.cpp,
// source/levelset.cpp.  The formulation is stated in DESIGN.md ("Particle resampling").
#include "common.h"
#include "../../include/manta_hip_resample.h"
#include "scan.h"

using namespace mf;

namespace {

constexpr int PNEW_ = 1, PDELETE_ = 1 << 10;
// class of a particle in one round: not looked at (deleted already), killed whatever its cell holds, surface, normal
constexpr int C_SKIP = 0, C_KILL = 1, C_SURF = 2, C_NORM = 3;

// this file's per-device scratch (arena_reserve): the working arrays of a round and the compress plan, which stays in the block
// between a round and its moves -- no other entry may take the block over.  Grows geometrically, never shrinks.
Arena g_arena[MAX_DEVICES];
struct Plan {
	int32_t *holes, *fillers;   // the current compress plan, inside the block
};
Plan g_plan[MAX_DEVICES];
// the block of `need` bytes and the device's plan; the plan of a block that had to be regrown is gone with it
static int arena(size_t need, Arena** out, Plan** plan) {
	bool regrown = false;
	const int rc = arena_reserve(g_arena, need, out, &regrown);
	if (regrown) g_plan[*out - g_arena] = Plan{nullptr, nullptr};   // also where the new allocation failed
	if (rc) return rc;
	*plan = &g_plan[*out - g_arena];
	return 0;
}

// ---- grid operations ---------------------------------------------------------------------------------------------------------
// knSetBoundaryNeumann, grid.cpp:640-669: the source cell lies strictly inside (the entry checks the sizes), so no thread reads a
// cell another one writes
__global__ __launch_bounds__(BLOCK) void k_set_bound_neumann(Dim d, uint32_t* __restrict__ g, int w) {
	CELL_IJK(d)
	int si = i, sj = j, sk = k;
	bool set = false;
	if (i <= w) { si = w + 1; set = true; }
	if (i >= d.sx - 1 - w) { si = d.sx - 1 - w - 1; set = true; }
	if (j <= w) { sj = w + 1; set = true; }
	if (j >= d.sy - 1 - w) { sj = d.sy - 1 - w - 1; set = true; }
	if (d.is3d) {
		if (k <= w) { sk = w + 1; set = true; }
		if (k >= d.sz - 1 - w) { sk = d.sz - 1 - w - 1; set = true; }
	}
	if (set) g[idx] = g[(int64_t)si + d.Y * sj + d.Z * sk];
}

// LevelsetGrid::initFromFlags, levelset.cpp:231-238
__global__ __launch_bounds__(BLOCK) void k_init_from_flags(int64_t n, float* __restrict__ phi, const int32_t* __restrict__ flags,
                                                           int ignoreWalls) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	const int f = flags[idx];
	phi[idx] = ((f & MF_FLUID) || (ignoreWalls && (f & MF_OBSTACLE))) ? -0.5f : 0.5f;
}

// knCombineVels, plugin/flip.cpp:748-770
__global__ __launch_bounds__(BLOCK) void k_combine_vels(Dim d, float* __restrict__ vel, const float* __restrict__ w,
                                                        float* __restrict__ comb, const float* __restrict__ phi, float narrowBand,
                                                        float thresh) {
	CELL_IJK(d)
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const int64_t o = (int64_t)c * d.n + idx;
		if (phi) {
			float p[3] = {(float)i, (float)j, (float)k};
			p[(c + 1) % 3] += 0.5f;
			p[(c + 2) % 3] += 0.5f;
			if (interpol1(d, phi, p[0], p[1], p[2]) < -narrowBand) {
				vel[o] = 0.f;
				continue;
			}
		}
		if (w[o] > thresh) {
			comb[o] = vel[o];
			vel[o] = -1.f;
		} else {
			vel[o] = 0.f;
		}
	}
}

// ---- one round of adjustNumber's particle loop ----------------------------------------------------------------------------------
// plugin/flip.cpp:215-227 for the particle t = i0 + q: its class, its cell as the sort key (nc for the ones no cell counts), and
// the number of counted particles per cell
__global__ __launch_bounds__(BLOCK) void k_classify(Dim d, const float* __restrict__ phi, int64_t m, int64_t ps,
                                                    const float* __restrict__ pos, const int32_t* __restrict__ pflag, int64_t i0,
                                                    float narrowBand, float surfLs, int32_t* __restrict__ keys,
                                                    int32_t* __restrict__ vals, int32_t* __restrict__ cls, int32_t* __restrict__ cnt) {
	const int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (q >= m) return;
	const int64_t t = i0 + q;
	int key = (int)d.n, c = C_SKIP;
	if (!(pflag[t] & PDELETE_)) {
		const float x = pos[t], y = pos[ps + t], z = pos[2 * ps + t];
		const int ix = (int)x, iy = (int)y, iz = (int)z;   // toVec3i: truncation
		c = C_KILL;
		if (ix >= 0 && iy >= 0 && iz >= 0 && ix < d.sx && iy < d.sy && iz < d.sz) {
			const float phiv = interpol1(d, phi, x, y, z);
			if (!(phiv > 0.f) && !(narrowBand > 0.f && phiv < -narrowBand)) {
				c = phiv > surfLs ? C_SURF : C_NORM;
				key = (int)((int64_t)ix + d.Y * iy + d.Z * iz);
				atomicAdd(&cnt[key], 1);
			}
		}
	}
	keys[q] = key;
	vals[q] = (int32_t)q;
	cls[q] = c;
}

// p-th entry of the cell-sorted (stable in particle index) list: f = tmp(cell) + counted particles before it in the cell; a normal
// particle is culled iff f > maxParticles (flip.cpp:228-235).  cls becomes the kill decision in bit 2.
__global__ __launch_bounds__(BLOCK) void k_decide(int64_t m, int nc, const int32_t* __restrict__ skeys,
                                                  const int32_t* __restrict__ svals, const int32_t* __restrict__ start,
                                                  const int32_t* __restrict__ tmp, int maxParticles, const int32_t* __restrict__ cls,
                                                  int32_t* __restrict__ kill) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= m) return;
	const int key = skeys[p], q = svals[p], c = cls[q];
	int kl;
	if (key == nc)
		kl = c == C_KILL;
	else
		kl = c == C_NORM && tmp[key] + ((int)p - start[key]) > maxParticles;
	kill[q] = kl;
}

// the first kill whose running count passes the chunk: the one the serial loop compresses at (particle.h:426)
__global__ __launch_bounds__(BLOCK) void k_find(int64_t m, const int32_t* __restrict__ kill, const int32_t* __restrict__ pre,
                                                int64_t md, int64_t chunk, int64_t* __restrict__ res) {
	const int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (q >= m || !kill[q]) return;
	const int64_t c = md + pre[q];
	if (c > chunk && (c - 1 <= chunk || pre[q] == 1)) res[0] = q;   // exactly one thread
}

// kills and counts of the particles up to and including the hit (all of them without one)
__global__ __launch_bounds__(BLOCK) void k_apply(int64_t m, int64_t i0, const int32_t* __restrict__ keys,
                                                 const int32_t* __restrict__ cls, const int32_t* __restrict__ kill,
                                                 const int32_t* __restrict__ pre, int64_t* __restrict__ res,
                                                 int32_t* __restrict__ pflag, int32_t* __restrict__ tmp) {
	const int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (q >= m) return;
	const int64_t hit = res[0];
	const int64_t last = hit >= 0 ? hit : m - 1;
	if (q > last) return;
	if (q == last) res[1] = pre[q];
	if (kill[q])
		pflag[i0 + q] |= PDELETE_;
	else if (cls[q] >= C_SURF)
		atomicAdd(&tmp[keys[q]], 1);
}
// idx* in particle indices
__global__ void k_round_finish(int64_t i0, int64_t np, int64_t* res) {
	if (res[0] >= 0)
		res[0] += i0;
	else {
		res[2] = np;
		res[3] = 0;
	}
}

// ---- compress -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_alive(int64_t np, const int32_t* __restrict__ pflag, int32_t* __restrict__ alive) {
	const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (i < np) alive[i] = (pflag[i] & PDELETE_) ? 0 : 1;
}
// A: exclusive prefix of alive.  M = A[np-1] + alive[np-1]; hole i (deleted, i < M) has rank i - A[i]; filler i (kept, i >= M) has
// the rank "kept slots after it" = M - A[i] - 1.  res[2] = M, res[3] = holes (when `active` allows: a round without a hit keeps its own)
__global__ __launch_bounds__(BLOCK) void k_plan(int64_t np, const int32_t* __restrict__ pflag, const int32_t* __restrict__ A,
                                                int32_t* __restrict__ holes, int32_t* __restrict__ fillers, int64_t* __restrict__ res,
                                                int needs_hit) {
	const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (i >= np) return;
	if (needs_hit && res[0] < 0) return;
	const int64_t M = (int64_t)A[np - 1] + ((pflag[np - 1] & PDELETE_) ? 0 : 1);
	const bool dead = pflag[i] & PDELETE_;
	if (i < M && dead) holes[i - A[i]] = (int32_t)i;
	if (i >= M && !dead) fillers[M - A[i] - 1] = (int32_t)i;
	if (i == 0) {
		res[2] = M;
		if (M == np) res[3] = 0;
	}
	if (i == M) res[3] = M - A[M];
}
__global__ __launch_bounds__(BLOCK) void k_move(int64_t H, const int32_t* __restrict__ holes, const int32_t* __restrict__ fillers,
                                                int ncomp, int64_t ps, uint32_t* __restrict__ data) {
	const int64_t k = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (k >= H) return;
	const int64_t h = holes[k], f = fillers[k];
	for (int c = 0; c < ncomp; c++) data[c * ps + h] = data[c * ps + f];
}

static int plan_launch(Plan* plan, int64_t np, const int32_t* pflag, int32_t* A, int32_t* holes, int32_t* fillers, void* cub,
                       size_t cub_bytes, int64_t* res, int needs_hit, hipStream_t st) {
	hipLaunchKernelGGL(k_alive, dim3(nblk(np)), dim3(BLOCK), 0, st, np, pflag, A);
	MF_TRY(exclusive_sum(cub, cub_bytes, A, A, np, st));
	hipLaunchKernelGGL(k_plan, dim3(nblk(np)), dim3(BLOCK), 0, st, np, pflag, A, holes, fillers, res, needs_hit);
	MF_LAUNCH_CHECK();
	plan->holes = holes;
	plan->fillers = fillers;
	return 0;
}

// ---- seeding ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_clear_new(int64_t np, int32_t* __restrict__ pflag) {
	const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (i < np) pflag[i] &= ~PNEW_;
}
// plugin/flip.cpp:241-250
__global__ __launch_bounds__(BLOCK) void k_seed_need(int64_t n, const int32_t* __restrict__ flags, const float* __restrict__ phi,
                                                     const float* __restrict__ exclude, const int32_t* __restrict__ tmp, int minP,
                                                     float narrowBand, float surfLs, int32_t* __restrict__ need) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	const float p = phi[idx];
	int nd = 0;
	const bool skip = p > surfLs || (narrowBand > 0.f && p < -narrowBand) || (exclude && exclude[idx] < 0.f);
	if (!skip && (flags[idx] & MF_FLUID)) {
		nd = minP - tmp[idx];
		if (nd < 0) nd = 0;
	}
	need[idx] = nd;
}
__global__ void k_seed_total(int64_t n, const int32_t* need, const int32_t* offsets, int64_t* res) {
	res[0] = (int64_t)offsets[n - 1] + need[n - 1];
}
// plugin/flip.cpp:250-256 + particle.h:645-650
__global__ __launch_bounds__(BLOCK) void k_seed_insert(Dim d, const int32_t* __restrict__ offsets, const float* __restrict__ reals,
                                                       int64_t np, int64_t total, int64_t ps, float* __restrict__ pos,
                                                       int32_t* __restrict__ pflag) {
	CELL_IJK(d)
	const int64_t first = offsets[idx];
	const int64_t end = idx + 1 < d.n ? (int64_t)offsets[idx + 1] : total;
	for (int64_t m = first; m < end; m++) {
		const float* r = reals + 3 * m;
		const int64_t s = np + m;
		pos[s] = (float)i + r[0];
		pos[ps + s] = (float)j + r[1];
		pos[2 * ps + s] = d.is3d ? (float)k + r[2] : 0.5f;
		pflag[s] = PNEW_;
	}
}

// ParticleDataImpl<T>::initNewValue, particle.cpp:348-369
__global__ __launch_bounds__(BLOCK) void k_pdata_init(Dim d, const float* __restrict__ grid, int mode, int ncomp, int64_t first,
                                                      int64_t count, int64_t ps, const float* __restrict__ pos,
                                                      float* __restrict__ data) {
	const int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (q >= count) return;
	const int64_t t = first + q;
	if (mode == 0) {
		for (int c = 0; c < ncomp; c++) data[c * ps + t] = 0.f;   // the all-zero word, for int channels as well
		return;
	}
	const float x = pos[t], y = pos[ps + t], z = pos[2 * ps + t];
	if (mode == 2) {
		float vx, vy, vz;
		interpol_mac(d, grid, x, y, z, vx, vy, vz);
		data[t] = vx;
		data[ps + t] = vy;
		data[2 * ps + t] = vz;
	} else {
		for (int c = 0; c < ncomp; c++) data[c * ps + t] = interpol1(d, grid + (int64_t)c * d.n, x, y, z);
	}
}

}  // namespace

extern "C" {

int mf_resample_abi_version(void) { return MF_RESAMPLE_ABI_VERSION; }

int mf_grid_set_bound_neumann(int sx, int sy, int sz, void* data, int boundaryWidth, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	const int w = boundaryWidth, lo = 2 * w + 3;
	if (w < 0) return fail("setBoundNeumann: boundaryWidth %d < 0", w);
	if (sx < lo || sy < lo || (d.is3d && sz < lo))
		return fail("setBoundNeumann: grid %dx%dx%d too small for boundaryWidth %d (needs %d cells per axis)", sx, sy, sz, w, lo);
	hipLaunchKernelGGL(k_set_bound_neumann, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, (uint32_t*)data, w);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_levelset_init_from_flags(int64_t n, float* phi, const int32_t* flags, int ignoreWalls, void* stream) {
	if (n <= 0) return 0;
	hipLaunchKernelGGL(k_init_from_flags, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, phi, flags, ignoreWalls);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_combine_grid_vel(int sx, int sy, int sz, float* vel, const float* weight, float* combineVel, const float* phi,
                        float narrowBand, float thresh, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_combine_vels, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, vel, weight, combineVel, phi,
	                   narrowBand, thresh);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_resample_round(int sx, int sy, int sz, const float* phi, int32_t* tmp, int64_t np, int64_t pstride, const float* pos,
                      int32_t* pflag, int64_t i0, int maxParticles, float narrowBand, float surfaceLs, int64_t mDeletes,
                      int64_t mDeleteChunk, int64_t* result_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	if (np >= ((int64_t)1 << 31)) return fail("adjustNumber: too many particles for 32-bit indices");
	if (i0 < 0 || i0 > np || pstride < np) return fail("adjustNumber: bad particle range (i0 %lld, np %lld, stride %lld)", (long long)i0, (long long)np, (long long)pstride);
	const int64_t m = np - i0;
	if (m == 0) {
		result_host[0] = -1;
		result_host[1] = 0;
		result_host[2] = np;
		result_host[3] = 0;
		return 0;
	}
	const int nc = (int)d.n, end_bit = key_bits(nc);
	// arena: 6 arrays of np words (keys, sorted keys, vals, sorted vals, cls, kill; the prefix reuses sorted keys, the plan reuses
	// keys / vals / sorted vals), cnt and start of nc + 1 words, the result block, the scan / sort workspace
	size_t cub_bytes = 0;
	MF_TRY(inclusive_sum32_bytes(m, &cub_bytes));
	MF_TRY(exclusive_sum32_bytes(nc + 1, &cub_bytes));
	MF_TRY(exclusive_sum32_bytes(np, &cub_bytes));
	MF_TRY(sort_pairs_bytes(m, end_bit, &cub_bytes));
	const size_t wp = al256(sizeof(int32_t) * (size_t)np), wc = al256(sizeof(int32_t) * ((size_t)nc + 1));
	const size_t need = 6 * wp + 2 * wc + 256 + al256(cub_bytes);
	Arena* a;
	Plan* plan;
	MF_TRY(arena(need, &a, &plan));
	Cutter c(a->p, need);
	int32_t *keys, *skeys, *vals, *svals, *cls, *kill, *cnt, *start;
	int64_t* res;
	char* cub;
	MF_TRY(c.take(np, &keys, &skeys, &vals, &svals, &cls, &kill));
	MF_TRY(c.take(nc + 1, &cnt, &start));
	MF_TRY(c.take(32, &res));
	MF_TRY(c.take(cub_bytes, &cub));
	int32_t* pre = skeys;   // free once k_decide has read the sorted keys

	MF_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * ((size_t)nc + 1), st));
	MF_HIP(hipMemsetAsync(res, 0xff, sizeof(int64_t), st));          // res[0] = -1
	MF_HIP(hipMemsetAsync(res + 1, 0, 3 * sizeof(int64_t), st));
	const dim3 gm(nblk(m)), bl(BLOCK);
	hipLaunchKernelGGL(k_classify, gm, bl, 0, st, d, phi, m, pstride, pos, pflag, i0, narrowBand, surfaceLs, keys, vals, cls, cnt);
	MF_TRY(exclusive_sum(cub, cub_bytes, cnt, start, nc + 1, st));
	MF_TRY(sort_pairs(cub, cub_bytes, (uint32_t*)keys, (uint32_t*)skeys, vals, svals, m, end_bit, st));
	hipLaunchKernelGGL(k_decide, gm, bl, 0, st, m, nc, skeys, svals, start, tmp, maxParticles, cls, kill);
	MF_TRY(inclusive_sum(cub, cub_bytes, kill, pre, m, st));
	hipLaunchKernelGGL(k_find, gm, bl, 0, st, m, kill, pre, mDeletes, mDeleteChunk, res);
	hipLaunchKernelGGL(k_apply, gm, bl, 0, st, m, i0, keys, cls, kill, pre, res, pflag, tmp);
	MF_LAUNCH_CHECK();
	// the plan of the whole array; its kernels do nothing when the round had no hit
	MF_TRY(plan_launch(plan, np, pflag, svals, keys, vals, cub, cub_bytes, res, 1, st));
	hipLaunchKernelGGL(k_round_finish, dim3(1), dim3(1), 0, st, i0, np, res);
	MF_LAUNCH_CHECK();
	return read_back(result_host, res, 4 * sizeof(int64_t), st);
}

int mf_particles_compress_plan(int64_t np, const int32_t* pflag, int64_t* result_host, void* stream) {
	hipStream_t st = (hipStream_t)stream;
	if (np <= 0) {
		result_host[0] = result_host[1] = 0;
		return 0;
	}
	if (np >= ((int64_t)1 << 31)) return fail("compress: too many particles for 32-bit indices");
	size_t scan_p = 0;
	MF_TRY(exclusive_sum32_bytes(np, &scan_p));
	const size_t need = 3 * al256(sizeof(int32_t) * (size_t)np) + 256 + al256(scan_p);
	Arena* a;
	Plan* plan;
	MF_TRY(arena(need, &a, &plan));
	Cutter c(a->p, need);
	int32_t *A, *holes, *fillers;
	int64_t* res;
	char* cub;
	MF_TRY(c.take(np, &A, &holes, &fillers));
	MF_TRY(c.take(32, &res));
	MF_TRY(c.take(scan_p, &cub));
	MF_HIP(hipMemsetAsync(res, 0, 4 * sizeof(int64_t), st));
	MF_TRY(plan_launch(plan, np, pflag, A, holes, fillers, cub, scan_p, res, 0, st));
	return read_back(result_host, res + 2, 2 * sizeof(int64_t), st);
}

int mf_particles_compress_move(int64_t holes, int ncomp, int64_t pstride, void* data, void* stream) {
	if (holes <= 0) return 0;
	Arena* a;
	Plan* plan;
	MF_TRY(arena(0, &a, &plan));
	if (!plan->holes) return fail("compress: no plan (mf_resample_round / mf_particles_compress_plan come first)");
	if (ncomp < 1 || ncomp > 3) return fail("compress: %d components", ncomp);
	hipLaunchKernelGGL(k_move, dim3(nblk(holes)), dim3(BLOCK), 0, (hipStream_t)stream, holes, plan->holes, plan->fillers, ncomp, pstride,
	                   (uint32_t*)data);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_resample_seed_plan(int sx, int sy, int sz, const int32_t* flags, const float* phi, const float* exclude, const int32_t* tmp,
                          int minParticles, float narrowBand, float surfaceLs, int64_t np, int32_t* pflag, int32_t* offsets,
                          int64_t* total_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	size_t scan_c = 0;
	MF_TRY(exclusive_sum32_bytes(d.n, &scan_c));
	const size_t need_bytes = al256(sizeof(int32_t) * (size_t)d.n) + 256 + al256(scan_c);
	// a compress plan is pending only between a round and its moves; seeding comes after them and takes the arena over
	Arena* a;
	Plan* plan;
	MF_TRY(arena(need_bytes, &a, &plan));
	plan->holes = plan->fillers = nullptr;
	Cutter c(a->p, need_bytes);
	int32_t* need;
	int64_t* res;
	char* cub;
	MF_TRY(c.take(d.n, &need));
	MF_TRY(c.take(32, &res));
	MF_TRY(c.take(scan_c, &cub));
	if (np > 0) hipLaunchKernelGGL(k_clear_new, dim3(nblk(np)), dim3(BLOCK), 0, st, np, pflag);
	hipLaunchKernelGGL(k_seed_need, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d.n, flags, phi, exclude, tmp, minParticles, narrowBand,
	                   surfaceLs, need);
	MF_TRY(exclusive_sum(cub, scan_c, need, offsets, d.n, st));
	hipLaunchKernelGGL(k_seed_total, dim3(1), dim3(1), 0, st, d.n, need, offsets, res);
	MF_LAUNCH_CHECK();
	return read_back(total_host, res, sizeof(int64_t), st);
}

int mf_resample_seed_insert(int sx, int sy, int sz, const int32_t* offsets, const float* reals, int64_t np, int64_t total,
                            int64_t pstride, float* pos, int32_t* pflag, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	if (total <= 0) return 0;
	if (pstride < np + total) return fail("adjustNumber: particle capacity %lld below %lld", (long long)pstride, (long long)(np + total));
	hipLaunchKernelGGL(k_seed_insert, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, offsets, reals, np, total, pstride, pos,
	                   pflag);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_pdata_init_new(int sx, int sy, int sz, const float* grid, int mode, int ncomp, int64_t first, int64_t count, int64_t pstride,
                      const float* pos, void* data, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	if (count <= 0) return 0;
	if (mode < 0 || mode > 2 || (mode && !grid) || (mode == 2 && ncomp != 3) || (ncomp != 1 && ncomp != 3))
		return fail("pdata init: bad mode %d / components %d", mode, ncomp);
	if (first < 0 || first + count > pstride) return fail("pdata init: range past the capacity");
	hipLaunchKernelGGL(k_pdata_init, dim3(nblk(count)), dim3(BLOCK), 0, (hipStream_t)stream, d, grid, mode, ncomp, first, count,
	                   pstride, pos, (float*)data);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
