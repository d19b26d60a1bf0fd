// reinit.hip -- level-set reinitialisation by fast marching (include/open/manta_hip_reinit.h): the set-up passes and the seeding with one
// thread per cell, the march as windows of keys that pop in sub-rounds of mutually distant cells (a min-reduction per window; a selecting
// and a popping launch per sub-round, so that no entry sees a neighbour that pops in its own launch as popped), the heap as an unordered
// list of cells with an atomic counter, and the literal serial loop on the host for a march that cannot be proven exact.  The per-item
// bodies are in reinit_cells.h.  Reference: levelset.cpp:32-85, 122-228, fastmarch.cpp:23-221.
#include "reinit_cells.h"
#include "../../include/open/manta_hip_reinit.h"

using namespace mf;
using namespace mf::reinit;

namespace {

// ctr: 0 list length, 1 live entries, 2 ~(ordered bits) of the smallest key (0: none), 3 window entries left, 4 selected, 5 cells that
// went on the heap inside the window, 6 flag
enum { C_COUNT = 0, C_LIVE, C_MIN, C_NW, C_NSEL, C_JOIN, C_FLAG, C_WORDS = 8 };

// monotone map of the march-order key (time * dir) to unsigned, inverted so that the smallest key is the largest word
__device__ __forceinline__ uint32_t key_word(int dir, float t) {
	const uint32_t u = __float_as_uint(dir > 0 ? t : -t);
	return ~((u >> 31) ? ~u : (u | 0x80000000u));
}
__device__ __forceinline__ float word_key(int dir, uint32_t w) {
	const uint32_t e = ~w;
	const float s = __uint_as_float((e >> 31) ? (e ^ 0x80000000u) : ~e);
	return dir > 0 ? s : -s;
}

__global__ void __launch_bounds__(BLOCK) k_reinit_init(March m) {
	CELL_IJK(m.d)
	init_fm(m, idx, i, j, k);
}

__global__ void __launch_bounds__(BLOCK) k_reinit_seed(March m, int outer, int32_t* __restrict__ list, int32_t* __restrict__ ctr) {
	CELL_IJK(m.d)
	if (outer ? seed_outer(m, idx, i, j, k) : seed_interface(m, idx, i, j, k)) {
		const int pos = atomicAdd(&ctr[C_COUNT], 1);
		if (pos < m.d.n) list[pos] = (int32_t)idx;
	}
}

// the smallest key of the entries still on the heap, and their number
__global__ void __launch_bounds__(BLOCK) k_reinit_min(March m, const int32_t* __restrict__ list, int32_t* __restrict__ ctr) {
	const int64_t e = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	uint32_t w = 0;
	int live = 0;
	if (e < ctr[C_COUNT] && e < m.d.n) {
		const int64_t c = list[e];
		if (m.fm[c] == FM_ONHEAP) {
			w = key_word(m.dir, m.key[c]);
			live = 1;
		}
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const uint32_t w2 = __shfl_xor(w, o, 64);
		w = w2 > w ? w2 : w;
		live += __shfl_xor(live, o, 64);
	}
	if ((threadIdx.x & 63) == 0 && live) {
		atomicMax((uint32_t*)&ctr[C_MIN], w);
		atomicAdd(&ctr[C_LIVE], live);
	}
}

// sub-round, first launch: the window entries that no earlier window entry within L1 distance 2 holds back
__global__ void __launch_bounds__(BLOCK)
k_reinit_select(March m, int w, const int32_t* __restrict__ list, int32_t* __restrict__ sel, int32_t* __restrict__ ctr) {
	const int64_t e = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (e >= ctr[C_COUNT] || e >= m.d.n || ctr[C_MIN] == 0) return;
	const float te = window_end(m.dir, word_key(m.dir, (uint32_t)ctr[C_MIN]));
	const int64_t c = list[e];
	if (m.fm[c] != FM_ONHEAP || !in_window(m.dir, m.key[c], te)) return;
	atomicAdd(&ctr[C_NW], 1);
	if (!selectable(m, c, te)) return;
	m.epoch[c] = w;
	const int pos = atomicAdd(&ctr[C_NSEL], 1);
	if (pos < m.d.n) sel[pos] = (int32_t)c;
}

struct DevicePush {
	March m;
	int32_t* list;
	int32_t* ctr;
	float te;
	int w;
	__device__ void operator()(int64_t q) const {
		const int pos = atomicAdd(&ctr[C_COUNT], 1);
		if (pos < m.d.n) list[pos] = (int32_t)q;
		if (in_window(m.dir, m.key[q], te)) atomicAdd(&ctr[C_JOIN], 1);      // it joins the window
		if (late_conflict(m, q, w)) atomicOr(&ctr[C_FLAG], 1);               // a neighbour popped that the serial loop pops after it
	}
};

// sub-round, second launch: the selected entries pop.  They lie more than 2 apart, so their write sets are disjoint and none reads
// what another writes
__global__ void __launch_bounds__(BLOCK)
k_reinit_pop(March m, int w, int32_t* __restrict__ list, const int32_t* __restrict__ sel, int32_t* __restrict__ ctr) {
	const int64_t e = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (e >= ctr[C_NSEL] || e >= m.d.n) return;
	const DevicePush push = {m, list, ctr, window_end(m.dir, word_key(m.dir, (uint32_t)ctr[C_MIN])), w};
	pop_cell(m, sel[e], push);
}

__global__ void __launch_bounds__(BLOCK) k_reinit_bnd_value(Dim d, const float* __restrict__ phi, float* __restrict__ tmp) {
	CELL_IJK(d)
	if (!interior(d, i, j, k)) tmp[idx] = boundary_value(d, phi, i, j, k);
}
__global__ void __launch_bounds__(BLOCK) k_reinit_bnd_store(Dim d, float* __restrict__ phi, const float* __restrict__ tmp) {
	CELL_IJK(d)
	if (!interior(d, i, j, k)) phi[idx] = tmp[idx];
}

__global__ void __launch_bounds__(BLOCK) k_reinit_uninit(March m, float val) {
	CELL_IJK(m.d)
	set_uninitialized(m, idx, i, j, k, val);
}

int check_grid(const char* who, int sx, int sy, int sz, bool device) {
	MF_TRY(check_dim(sx, sy, sz));
	if (sx < 3 || sy < 3 || (sz != 1 && sz < 3)) return fail("%s: a grid of %dx%dx%d has no interior", who, sx, sy, sz);
	if (device && g_slab_gsz > 0) return fail("%s: not available inside a z-slab window", who);
	return 0;
}

// the march that could not be proven exact (or was asked for): the three grids as they were at its start go down, the literal loop
// runs, they come up again with the keys
int serial_fallback(const March& m, int outer, const float* snapPhi, const int32_t* snapFm, const float* snapVel, int64_t* pops, hipStream_t st) {
	const int64_t n = m.d.n;
	std::vector<float> phi(n), key(n, 0.f), vel(m.vel ? 3 * n : 0);
	std::vector<int32_t> fm(n), flags(n);
	MF_HIP(hipMemcpyAsync(phi.data(), snapPhi, n * sizeof(float), hipMemcpyDeviceToHost, st));
	MF_HIP(hipMemcpyAsync(fm.data(), snapFm, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	MF_HIP(hipMemcpyAsync(flags.data(), m.flags, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	if (m.vel) MF_HIP(hipMemcpyAsync(vel.data(), snapVel, 3 * n * sizeof(float), hipMemcpyDeviceToHost, st));
	MF_HIP(hipStreamSynchronize(st));
	March h = m;
	h.phi = phi.data();
	h.fm = fm.data();
	h.key = key.data();
	h.fm0 = fm.data();
	h.flags = flags.data();
	h.vel = m.vel ? vel.data() : nullptr;
	h.epoch = nullptr;
	*pops = serial_march(h, outer != 0);
	MF_HIP(hipMemcpyAsync(m.phi, phi.data(), n * sizeof(float), hipMemcpyHostToDevice, st));
	MF_HIP(hipMemcpyAsync(m.fm, fm.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, st));
	MF_HIP(hipMemcpyAsync(m.key, key.data(), n * sizeof(float), hipMemcpyHostToDevice, st));
	if (m.vel) MF_HIP(hipMemcpyAsync(m.vel, vel.data(), 3 * n * sizeof(float), hipMemcpyHostToDevice, st));
	MF_HIP(hipStreamSynchronize(st));
	return 0;
}

}  // namespace

extern "C" {

int mf_reinit_abi_version(void) { return MF_REINIT_ABI_VERSION; }

int mf_reinit_march(int sx, int sy, int sz, float* phi, const int32_t* flags, float* vel, int32_t* fm, float* key, int32_t* list, int32_t* sel,
                    int32_t* epoch, float* snapPhi, int32_t* snapFm, float* snapVel, int32_t* ctr, float maxTime, int dir, int ignoreWalls, int correctOuterLayer,
                    int obstacleType, int serial, int64_t* stats_host, void* stream) {
	MF_TRY(check_grid("reinitMarching", sx, sy, sz, true));
	if (dir != 1 && dir != -1) return fail("reinitMarching: direction %d", dir);
	if (dir < 0) vel = nullptr;
	if (vel && !snapVel) return fail("reinitMarching: velocity transport needs its scratch grid");
	const Dim d = mkdim(sx, sy, sz);
	const hipStream_t st = (hipStream_t)stream;
	const int outer = dir > 0 && correctOuterLayer;
	const dim3 cells(nblk(d.n)), blk(BLOCK);
	March m = {d, phi, fm, key, fm, flags, vel, maxTime * (float)dir, dir, ignoreWalls != 0, obstacleType, epoch};
	int64_t windows = 0, subrounds = 0, pops = 0, launches = 0, readbacks = 0;
	hipLaunchKernelGGL(k_reinit_init, cells, blk, 0, st, m);
	MF_LAUNCH_CHECK();
	launches++;
	MF_HIP(hipMemcpyAsync(snapPhi, phi, d.n * sizeof(float), hipMemcpyDeviceToDevice, st));
	MF_HIP(hipMemcpyAsync(snapFm, fm, d.n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
	if (vel) MF_HIP(hipMemcpyAsync(snapVel, vel, 3 * d.n * sizeof(float), hipMemcpyDeviceToDevice, st));
	m.fm0 = snapFm;
	bool flagged = serial != 0;
	if (!flagged) {
		int32_t host[C_WORDS] = {0};
		MF_HIP(hipMemsetAsync(ctr, 0, C_WORDS * sizeof(int32_t), st));
		hipLaunchKernelGGL(k_reinit_seed, cells, blk, 0, st, m, outer, list, ctr);
		MF_LAUNCH_CHECK();
		launches++;
		MF_TRY(read_back(host, ctr, sizeof(host), st));
		readbacks++;
		int64_t count = host[C_COUNT];
		for (bool done = count == 0; !done && !flagged;) {
			MF_HIP(hipMemsetAsync(ctr + C_LIVE, 0, 2 * sizeof(int32_t), st));
			hipLaunchKernelGGL(k_reinit_min, dim3(nblk(count)), blk, 0, st, m, (const int32_t*)list, ctr);
			launches++;
			for (bool first = true;; first = false) {
				MF_HIP(hipMemsetAsync(ctr + C_NW, 0, 3 * sizeof(int32_t), st));
				hipLaunchKernelGGL(k_reinit_select, dim3(nblk(count)), blk, 0, st, m, (int)(windows + first), (const int32_t*)list, sel, ctr);
				hipLaunchKernelGGL(k_reinit_pop, dim3(nblk(count)), blk, 0, st, m, (int)(windows + first), list, (const int32_t*)sel, ctr);
				MF_LAUNCH_CHECK();
				launches += 2;
				MF_TRY(read_back(host, ctr, sizeof(host), st));
				readbacks++;
				if (host[C_LIVE] == 0) {
					done = true;
					break;
				}
				if (first) windows++;
				// no entry before the window's end (a key that is not a number), or a list that ran over: not provable
				if (host[C_NW] <= 0 || host[C_NSEL] <= 0 || host[C_COUNT] > d.n) {
					flagged = true;
					break;
				}
				subrounds++;
				pops += host[C_NSEL];
				count = host[C_COUNT];
				if (host[C_FLAG]) flagged = true;
				if (flagged || (host[C_NSEL] == host[C_NW] && host[C_JOIN] == 0)) break;
			}
		}
	}
	if (flagged) {
		windows = subrounds = 0;
		MF_TRY(serial_fallback(m, outer, snapPhi, snapFm, snapVel, &pops, st));
		readbacks += vel ? 4 : 3;
	} else {
		hipLaunchKernelGGL(k_reinit_bnd_value, cells, blk, 0, st, d, (const float*)phi, snapPhi);
		hipLaunchKernelGGL(k_reinit_bnd_store, cells, blk, 0, st, d, phi, (const float*)snapPhi);
		MF_LAUNCH_CHECK();
		launches += 2;
		MF_HIP(hipStreamSynchronize(st));
	}
	stats_host[0] = windows;
	stats_host[1] = subrounds;
	stats_host[2] = pops;
	stats_host[3] = flagged ? 1 : 0;
	stats_host[4] = launches;
	stats_host[5] = readbacks;
	return 0;
}

int mf_reinit_set_uninitialized(int sx, int sy, int sz, float* phi, const int32_t* fm, const int32_t* flags, float val, int ignoreWalls,
                                int obstacleType, void* stream) {
	MF_TRY(check_grid("reinitMarching", sx, sy, sz, true));
	const Dim d = mkdim(sx, sy, sz);
	const March m = {d, phi, const_cast<int32_t*>(fm), nullptr, fm, flags, nullptr, 0.f, 1, ignoreWalls != 0, obstacleType, nullptr};
	hipLaunchKernelGGL(k_reinit_uninit, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, m, val);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_reinit_march_serial(int sx, int sy, int sz, float* phi, int32_t* fm, float* key, const int32_t* flags, float* vel, float maxTime, int dir,
                           int ignoreWalls, int correctOuterLayer, int obstacleType, int64_t* pops_host) {
	MF_TRY(check_grid("reinitMarching", sx, sy, sz, false));
	if (dir != 1 && dir != -1) return fail("reinitMarching: direction %d", dir);
	Dim d = mkdim(sx, sy, sz);
	d.zoff = 0;
	d.gsz = sz;
	for (int64_t i = 0; i < d.n; i++) key[i] = 0.f;
	const March m = {d, phi, fm, key, fm, flags, dir > 0 ? vel : nullptr, maxTime * (float)dir, dir, ignoreWalls != 0, obstacleType, nullptr};
	*pops_host = serial_march(m, dir > 0 && correctOuterLayer);
	return 0;
}

}  // extern "C"
