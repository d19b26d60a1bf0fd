// surfturb.hip -- surface turbulence (include/open/manta_hip_surfturb.h): the cell lists as stable sorts of the slots by cell, and every
// stage of particleSurfaceTurbulence as one thread per point walking the cached lists in the reference's order.  The per-point bodies
// are in surfturb_cells.h.  Reference: plugin/surfaceturbulence.cpp.  Contract: DESIGN.md section 27.
#include "surfturb_cells.h"
#include "../../include/open/manta_hip_surfturb.h"
#include "scan.h"

using namespace mf;
using namespace mf::surfturb;

namespace {

__device__ __forceinline__ void store3(float* a, int64_t stride, int64_t i, V3 v) {
	a[i] = v.x;
	a[stride + i] = v.y;
	a[2 * stride + i] = v.z;
}

__global__ void __launch_bounds__(BLOCK) k_cell_keys(Par par, int R, Pts P, uint32_t* __restrict__ key, int32_t* __restrict__ val) {
	ITEM_IDX(P.n)
	key[idx] = (uint32_t)cell_of(pos_of(P, idx), par.res, R);
	val[idx] = (int32_t)idx;
}
// the sorted keys -> start[ncells + 1]: one thread per cell finds the first sorted slot whose cell is not below its own (a thread per
// slot filling the gap to the cell before it serialises on the long empty runs of a thin shell of points)
__global__ void __launch_bounds__(BLOCK) k_cell_starts(int64_t n, int64_t ncells, const uint32_t* __restrict__ key, int32_t* __restrict__ start) {
	ITEM_IDX(ncells + 1)
	int64_t lo = 0, hi = n;
	while (lo < hi) {
		const int64_t mid = (lo + hi) >> 1;
		if ((int64_t)key[mid] < idx) lo = mid + 1;
		else hi = mid;
	}
	start[idx] = (int32_t)lo;
}

__global__ void __launch_bounds__(BLOCK)
k_init_mark(Par par, Cells CC, Pts coarse, int sx, int sy, int sz, const int32_t* __restrict__ gridflags, int64_t ndirs, const float* __restrict__ dirs,
            int32_t* __restrict__ mark) {
	ITEM_IDX(coarse.n * ndirs)
	const int64_t p = idx / ndirs, d = idx % ndirs;
	V3 out;
	mark[idx] = init_fine(par, CC, coarse, sx, sy, sz, gridflags, p, V3{dirs[3 * d], dirs[3 * d + 1], dirs[3 * d + 2]}, out);
}
__global__ void __launch_bounds__(BLOCK)
k_init_fill(Par par, Pts coarse, int64_t ndirs, const float* __restrict__ dirs, const int32_t* __restrict__ mark, int64_t cap, float* __restrict__ pos,
            int32_t* __restrict__ flag) {
	ITEM_IDX(coarse.n * ndirs)
	const int32_t below = idx ? mark[idx - 1] : 0;
	if (mark[idx] == below) return;
	const int64_t p = idx / ndirs, d = idx % ndirs;
	store3(pos, cap, below, pos_of(coarse, p) + par.outerRadius * V3{dirs[3 * d], dirs[3 * d + 1], dirs[3 * d + 2]});
	flag[below] = 0;
}

__global__ void __launch_bounds__(BLOCK) k_advect(Par par, Cells CP, Pts prev, Pts coarse, Pts surf, float* pos) {
	ITEM_IDX(surf.n)
	if (!active(surf, idx)) return;
	store3(pos, surf.cap, idx, advect_point(par, CP, prev, coarse, pos_of(surf, idx)));
}

__global__ void __launch_bounds__(BLOCK) k_add_mark(Par par, Cells CC, Pts coarse, Cells CS, Pts surf, float* __restrict__ cand, int32_t* __restrict__ mark) {
	ITEM_IDX(surf.n)
	V3 out;
	mark[idx] = add_candidate(par, CC, coarse, CS, surf, idx, out);
	store3(cand, surf.n, idx, out);
}
__global__ void __launch_bounds__(BLOCK)
k_add_apply(int64_t n, int64_t cap, float* __restrict__ pos, int32_t* __restrict__ flag, const float* __restrict__ cand, const int32_t* __restrict__ mark) {
	ITEM_IDX(n)
	flag[idx] &= ~PNEW;
	const int32_t below = idx ? mark[idx - 1] : 0;
	if (mark[idx] == below || n + below >= cap) return;
	store3(pos, cap, n + below, vec_of(cand, n, idx));
	flag[n + below] = PNEW;
}

__global__ void __launch_bounds__(BLOCK)
k_greedy(Par par, Cells CS, Pts surf, const int32_t* __restrict__ in, int32_t* __restrict__ out, int32_t* __restrict__ head) {
	ITEM_IDX(surf.n)
	int32_t s = in[idx];
	if (s == 0) {
		s = greedy_decide(par, CS, surf, in, idx);
		if (s == 0) head[0] = 1;
	}
	out[idx] = s;
}
__global__ void __launch_bounds__(BLOCK)
k_delete(Par par, Cells CC, Pts coarse, Pts surf, int32_t* flag, const int32_t* __restrict__ state, int32_t* __restrict__ head) {
	ITEM_IDX(surf.n)
	const int r = delete_coarse(par, CC, coarse, pos_of(surf, idx));
	const int k1 = state[idx] == 2;
	if (k1) atomicAdd(&head[0], 1);
	if (r & 1) atomicAdd(&head[1], 1);
	if (r & 2) atomicAdd(&head[2], 1);
	if (k1 || r) flag[idx] |= PDELETE;
}
__global__ void __launch_bounds__(BLOCK) k_clear_new(int64_t n, int32_t* __restrict__ flag) {
	ITEM_IDX(n)
	flag[idx] &= ~PNEW;
}

__global__ void __launch_bounds__(BLOCK) k_normals(Par par, Cells CC, Pts coarse, Cells CS, Pts surf, float* __restrict__ normals) {
	ITEM_IDX(surf.n)
	store3(normals, surf.cap, idx, surface_normal(par, CC, coarse, CS, surf, idx));
}
__global__ void __launch_bounds__(BLOCK) k_avg_normals(Par par, Cells CS, Pts surf, const float* __restrict__ normals, float* __restrict__ tempv) {
	ITEM_IDX(surf.n)
	store3(tempv, surf.n, idx, averaged_normal(par, CS, surf, normals, idx));
}
// dst[3][dcap] (+)= src[3][n]
template <bool ADD>
__global__ void __launch_bounds__(BLOCK) k_assign3(int64_t n, int64_t dcap, float* __restrict__ dst, const float* __restrict__ src) {
	ITEM_IDX(n)
	for (int c = 0; c < 3; c++) dst[c * dcap + idx] = ADD ? dst[c * dcap + idx] + src[c * n + idx] : src[c * n + idx];
}
__global__ void __launch_bounds__(BLOCK) k_density(Par par, Cells CS, Pts surf, float* __restrict__ tempf) {
	ITEM_IDX(surf.n)
	tempf[idx] = surface_density(par, CS, surf, idx);
}
__global__ void __launch_bounds__(BLOCK)
k_displacement(Par par, Cells CS, Pts surf, const float* __restrict__ normals, const float* __restrict__ tempf, float* __restrict__ tempv) {
	ITEM_IDX(surf.n)
	store3(tempv, surf.n, idx, surface_displacement(par, CS, surf, normals, tempf, idx));
}
__global__ void __launch_bounds__(BLOCK) k_constrain(Par par, Cells CC, Pts coarse, Pts surf, float* pos) {
	ITEM_IDX(surf.n)
	store3(pos, surf.cap, idx, constrained(par, CC, coarse, pos_of(surf, idx)));
}

__global__ void __launch_bounds__(BLOCK) k_add_seed(int64_t n, float* __restrict__ H, const float* __restrict__ seed) {
	ITEM_IDX(n)
	H[idx] += seed[idx];
}
__global__ void __launch_bounds__(BLOCK)
k_wave_normal(Par par, Cells CS, Pts surf, const float* __restrict__ normals, const float* __restrict__ H, float* __restrict__ tempv) {
	ITEM_IDX(surf.n)
	store3(tempv, surf.n, idx, wave_normal(par, CS, surf, normals, H, idx));
}
__global__ void __launch_bounds__(BLOCK)
k_wave_laplacian(Par par, Cells CS, Pts surf, const float* __restrict__ normals, const float* __restrict__ H, const float* __restrict__ tempv,
                 float* __restrict__ tempf) {
	ITEM_IDX(surf.n)
	tempf[idx] = wave_laplacian(par, CS, surf, normals, H, tempv, idx);
}
__global__ void __launch_bounds__(BLOCK)
k_evolve(Par par, int64_t n, float* __restrict__ H, float* __restrict__ DtH, const float* __restrict__ seed, const float* __restrict__ tempf) {
	ITEM_IDX(n)
	float h = H[idx], d = DtH[idx];
	evolve_wave(par, tempf[idx], seed[idx], h, d);
	H[idx] = h;
	DtH[idx] = d;
}
__global__ void __launch_bounds__(BLOCK) k_curvature(Par par, Cells CS, Pts surf, const float* __restrict__ normals, float* __restrict__ tempf) {
	ITEM_IDX(surf.n)
	tempf[idx] = surface_curvature(par, CS, surf, normals, idx);
}
__global__ void __launch_bounds__(BLOCK) k_smooth_curvature(Par par, Cells CS, Pts surf, const float* __restrict__ tempf, float* __restrict__ source) {
	ITEM_IDX(surf.n)
	source[idx] = smooth_curvature(par, CS, surf, tempf, idx);
}
__global__ void __launch_bounds__(BLOCK) k_seed(Par par, int64_t n, float* __restrict__ source, float* __restrict__ seed, float* __restrict__ amp) {
	ITEM_IDX(n)
	float so = source[idx], se = seed[idx], a = amp[idx];
	seed_wave(par, so, se, a);
	source[idx] = so;
	seed[idx] = se;
	amp[idx] = a;
}

__global__ void __launch_bounds__(BLOCK) k_save_prev(Pts coarse, int64_t pcap, float* __restrict__ prev) {
	ITEM_IDX(coarse.n)
	if ((coarse.flag[idx] & (PNEW | PDELETE)) == 0) store3(prev, pcap, idx, pos_of(coarse, idx));
}
__global__ void __launch_bounds__(BLOCK) k_live_mark(int64_t n, const int32_t* __restrict__ flag, int32_t* __restrict__ mark) {
	ITEM_IDX(n)
	mark[idx] = (flag[idx] & PDELETE) == 0 ? 1 : 0;
}
__global__ void __launch_bounds__(BLOCK)
k_displaced(Pts surf, const float* __restrict__ normals, const float* __restrict__ H, const int32_t* __restrict__ mark, int64_t ocap, float* __restrict__ out,
            int32_t* __restrict__ oflag) {
	ITEM_IDX(surf.n)
	if (!active(surf, idx)) return;
	const int32_t r = mark[idx] - 1;
	store3(out, ocap, r, pos_of(surf, idx) + vec_of(normals, surf.cap, idx) * H[idx]);
	oflag[r] = 0;
}
__global__ void __launch_bounds__(BLOCK) k_check_parts(int sx, int sy, int sz, int64_t n, int64_t cap, const float* __restrict__ pos, int32_t* __restrict__ head) {
	ITEM_IDX(n)
	// toVec3i truncates; FlagGrid::isInBounds(p) with no boundary
	const int x = cvt_x86(pos[idx]), y = cvt_x86(pos[cap + idx]), z = cvt_x86(pos[2 * cap + idx]);
	if (x < 0 || y < 0 || z < 0 || x >= sx || y >= sy || z >= sz) atomicMin(&head[0], (int32_t)idx);
}
__global__ void k_set_i32(int32_t* p, int32_t a, int32_t b, int32_t c) {
	if (blockIdx.x || threadIdx.x) return;
	p[0] = a;
	p[1] = b;
	p[2] = c;
}

int check_set(const char* who, int64_t n, int64_t cap) {
	if (n < 0 || cap < n || n >= ((int64_t)1 << 31) - 1) return fail("%s: %lld points in arrays of stride %lld", who, (long long)n, (long long)cap);
	if (g_slab_gsz > 0) return fail("%s: not available inside a z-slab window", who);
	return 0;
}
int check_list(const char* who, int R) {
	if (R < 1 || (int64_t)R * R * R >= ((int64_t)1 << 31) - 1) return fail("%s: a cell list of resolution %d", who, R);
	return 0;
}
Par load_par(const float* par_host) {
	Par p;
	memcpy(&p, par_host, sizeof(p));
	return p;
}
// behind the head: keys and values, in and out, of the cell sort (n each), then the larger of the sort's and the scans' workspace
struct Tmp {
	uint32_t *k0, *k1;
	int32_t *v0, *v1;
	void* ws;
	size_t ws_bytes;
};
int64_t tmp_need(int64_t n, int64_t ncells, int64_t nscan) {
	size_t b = 0;
	if (n > 0) (void)sort_pairs_bytes(n, key_bits(ncells), &b);
	if (nscan > 0) (void)inclusive_sum32_bytes(nscan, &b);
	return head_ws_bytes(4 * al256(sizeof(int32_t) * (size_t)(n > 0 ? n : 1)) + b);
}
int tmp_cut(const char* who, void* tmp, int64_t tmp_bytes, int64_t n, int64_t ncells, int64_t nscan, Tmp* t) {
	HeadWs h;
	MF_TRY(head_ws_cut(who, tmp, tmp_bytes, tmp_need(n, ncells, nscan), &h));
	Cutter cut(h.ws, h.ws_bytes);
	const size_t m = (size_t)(n > 0 ? n : 1);
	MF_TRY(cut.take(m, &t->k0, &t->k1));
	MF_TRY(cut.take(m, &t->v0, &t->v1));
	t->ws = cut.p;
	t->ws_bytes = cut.left;
	return 0;
}
// the inclusive scan of mark[m] in place and its last entry to the host
int scan_total(const char* who, int32_t* mark, int64_t m, void* tmp, int64_t tmp_bytes, int64_t* total_host, hipStream_t st) {
	*total_host = 0;
	if (m == 0) return 0;
	Tmp t;
	MF_TRY(tmp_cut(who, tmp, tmp_bytes, 0, 1, m, &t));
	MF_TRY(inclusive_sum(t.ws, t.ws_bytes, mark, mark, m, st));
	int32_t total = 0;
	MF_TRY(read_back(&total, mark + (m - 1), sizeof(total), st));
	*total_host = total;
	return 0;
}

#define ST_LAUNCH(kernel, n, st, ...) hipLaunchKernelGGL(kernel, dim3(nblk(n)), dim3(BLOCK), 0, st, __VA_ARGS__)

}  // namespace

extern "C" {

int mf_surfturb_abi_version(void) { return MF_SURFTURB_ABI_VERSION; }

int mf_surfturb_params(int res, float outerRadius, int surfaceDensity, float dt, float waveSpeed, float waveDamping, float waveSeedFrequency,
                       float waveMaxAmplitude, float waveMaxFrequency, float waveMaxSeedingAmplitude, float curvCenter, float curvRadius,
                       float seedStep, int frameCount, float* par_host, int32_t* res_host) {
	if (res < 5 || !(outerRadius > 0.f) || surfaceDensity < 1)
		return fail("particleSurfaceTurbulence: res %d, outerRadius %g, surfaceDensity %d", res, (double)outerRadius, surfaceDensity);
	const Par p = derive_par(res, outerRadius, surfaceDensity, dt, waveSpeed, waveDamping, waveSeedFrequency, waveMaxAmplitude, waveMaxFrequency,
	                         waveMaxSeedingAmplitude, curvCenter, curvRadius, seedStep, frameCount);
	memcpy(par_host, &p, sizeof(p));
	res_host[0] = cvt_x86(2.f * res / p.outerRadius);
	res_host[1] = cvt_x86(1.f * res / (2.f * p.meanFineDistance));
	MF_TRY(check_list("particleSurfaceTurbulence", res_host[0]));
	return check_list("particleSurfaceTurbulence", res_host[1]);
}

int mf_surfturb_directions(const float* par_host, int64_t cap, float* dirs_host, int64_t* count_host) {
	const Par p = load_par(par_host);
	const int64_t count = direction_table(p, cap, dirs_host);
	if (count < 0) return fail("particleSurfaceTurbulence: more than 2^20 directions per coarse particle");
	*count_host = count;
	return 0;
}

int mf_surfturb_tmp_bytes(int64_t n, int64_t ncells, int64_t nscan, int64_t* bytes_host) {
	if (n < 0 || ncells < 1 || nscan < 0 || n >= ((int64_t)1 << 31) - 1 || ncells >= ((int64_t)1 << 31) - 1 || nscan >= ((int64_t)1 << 31) - 1)
		return fail("surface turbulence: %lld points, %lld cells, scans of %lld", (long long)n, (long long)ncells, (long long)nscan);
	*bytes_host = tmp_need(n, ncells, nscan);
	return 0;
}

int mf_surfturb_cells(const float* par_host, int R, int64_t n, int64_t cap, const float* pos, int32_t* start, int32_t* ids, void* tmp,
                      int64_t tmp_bytes, void* stream) {
	MF_TRY(check_set("surface turbulence cell list", n, cap));
	MF_TRY(check_list("surface turbulence cell list", R));
	const hipStream_t st = (hipStream_t)stream;
	const int64_t ncells = (int64_t)R * R * R;
	if (n == 0) {
		MF_HIP(hipMemsetAsync(start, 0, (ncells + 1) * sizeof(int32_t), st));
		return 0;
	}
	Tmp t;
	MF_TRY(tmp_cut("surface turbulence cell list", tmp, tmp_bytes, n, ncells, 0, &t));
	const Par par = load_par(par_host);
	const Pts P = {n, cap, pos, nullptr};
	ST_LAUNCH(k_cell_keys, n, st, par, R, P, t.k0, t.v0);
	MF_LAUNCH_CHECK();
	MF_TRY(sort_pairs(t.ws, t.ws_bytes, t.k0, t.k1, t.v0, t.v1, n, key_bits(ncells), st));
	ST_LAUNCH(k_cell_starts, ncells + 1, st, n, ncells, (const uint32_t*)t.k1, start);
	MF_LAUNCH_CHECK();
	MF_HIP(hipMemcpyAsync(ids, t.v1, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
	return 0;
}

int mf_surfturb_init_plan(const float* par_host, int sx, int sy, int sz, const int32_t* gridflags, int Rc, const int32_t* cstart,
                          const int32_t* cids, int64_t nc, int64_t ccap, const float* cpos, const int32_t* cflag, int64_t ndirs,
                          const float* dirs, int32_t* mark, void* tmp, int64_t tmp_bytes, int64_t* total_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	MF_TRY(check_set("particleSurfaceTurbulence", nc, ccap));
	MF_TRY(check_list("particleSurfaceTurbulence", Rc));
	if (ndirs < 0 || (ndirs > 0 && nc > (((int64_t)1 << 31) - 2) / ndirs)) return fail("particleSurfaceTurbulence: %lld particles times %lld directions", (long long)nc, (long long)ndirs);
	const hipStream_t st = (hipStream_t)stream;
	const int64_t m = nc * ndirs;
	*total_host = 0;
	if (m == 0) return 0;
	const Par par = load_par(par_host);
	const Cells CC = {Rc, cstart, cids};
	const Pts coarse = {nc, ccap, cpos, cflag};
	ST_LAUNCH(k_init_mark, m, st, par, CC, coarse, sx, sy, sz, gridflags, ndirs, dirs, mark);
	MF_LAUNCH_CHECK();
	return scan_total("particleSurfaceTurbulence", mark, m, tmp, tmp_bytes, total_host, st);
}

int mf_surfturb_init_fill(const float* par_host, int64_t nc, int64_t ccap, const float* cpos, int64_t ndirs, const float* dirs,
                          const int32_t* mark, int64_t cap, float* pos, int32_t* flag, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", nc, ccap));
	const int64_t m = nc * ndirs;
	if (m <= 0) return 0;
	const Pts coarse = {nc, ccap, cpos, nullptr};
	ST_LAUNCH(k_init_fill, m, (hipStream_t)stream, load_par(par_host), coarse, ndirs, dirs, mark, cap, pos, flag);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_surfturb_advect(const float* par_host, int Rc, const int32_t* pstart, const int32_t* pids, int64_t nc, int64_t ccap, const float* cpos,
                       const int32_t* cflag, int64_t pcap, const float* prev, int64_t n, int64_t cap, float* pos, const int32_t* flag,
                       void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, cap));
	MF_TRY(check_set("particleSurfaceTurbulence", nc, ccap < pcap ? ccap : pcap));
	MF_TRY(check_list("particleSurfaceTurbulence", Rc));
	if (n == 0) return 0;
	const Cells CP = {Rc, pstart, pids};
	const Pts pv = {nc, pcap, prev, nullptr}, coarse = {nc, ccap, cpos, cflag}, surf = {n, cap, pos, flag};
	ST_LAUNCH(k_advect, n, (hipStream_t)stream, load_par(par_host), CP, pv, coarse, surf, pos);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_surfturb_add_plan(const float* par_host, int Rc, const int32_t* cstart, const int32_t* cids, int64_t nc, int64_t ccap,
                         const float* cpos, const int32_t* cflag, int Rs, const int32_t* sstart, const int32_t* sids, int64_t n, int64_t cap,
                         const float* pos, const int32_t* flag, float* cand, int32_t* mark, void* tmp, int64_t tmp_bytes,
                         int64_t* total_host, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, cap));
	MF_TRY(check_set("particleSurfaceTurbulence", nc, ccap));
	MF_TRY(check_list("particleSurfaceTurbulence", Rc));
	MF_TRY(check_list("particleSurfaceTurbulence", Rs));
	const hipStream_t st = (hipStream_t)stream;
	*total_host = 0;
	if (n == 0) return 0;
	const Cells CC = {Rc, cstart, cids}, CS = {Rs, sstart, sids};
	const Pts coarse = {nc, ccap, cpos, cflag}, surf = {n, cap, pos, flag};
	ST_LAUNCH(k_add_mark, n, st, load_par(par_host), CC, coarse, CS, surf, cand, mark);
	MF_LAUNCH_CHECK();
	return scan_total("particleSurfaceTurbulence", mark, n, tmp, tmp_bytes, total_host, st);
}

int mf_surfturb_add_apply(int64_t n, int64_t total, int64_t cap, float* pos, int32_t* flag, const float* cand, const int32_t* mark, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, cap));
	if (total < 0 || total > n || n + total > cap) return fail("particleSurfaceTurbulence: %lld buffered points behind %lld in arrays of stride %lld", (long long)total, (long long)n, (long long)cap);
	if (n == 0) return 0;
	ST_LAUNCH(k_add_apply, n, (hipStream_t)stream, n, cap, pos, flag, cand, mark);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_surfturb_greedy_round(const float* par_host, int Rs, const int32_t* sstart, const int32_t* sids, int64_t n, int64_t cap,
                             const float* pos, const int32_t* flag, int first, int32_t* state_in, int32_t* state_out, int32_t* head,
                             int32_t* undecided_host, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, cap));
	MF_TRY(check_list("particleSurfaceTurbulence", Rs));
	*undecided_host = 0;
	if (n == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	const Cells CS = {Rs, sstart, sids};
	const Pts surf = {n, cap, pos, flag};
	MF_HIP(hipMemsetAsync(head, 0, sizeof(int32_t), st));
	if (first) MF_HIP(hipMemsetAsync(state_in, 0, n * sizeof(int32_t), st));
	ST_LAUNCH(k_greedy, n, st, load_par(par_host), CS, surf, (const int32_t*)state_in, state_out, head);
	MF_LAUNCH_CHECK();
	return read_back(undecided_host, head, sizeof(int32_t), st);
}

int mf_surfturb_delete(const float* par_host, int Rc, const int32_t* cstart, const int32_t* cids, int64_t nc, int64_t ccap, const float* cpos,
                       const int32_t* cflag, int64_t n, int64_t cap, const float* pos, int32_t* flag, const int32_t* state, int32_t* head,
                       int32_t* kills_host, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, cap));
	MF_TRY(check_set("particleSurfaceTurbulence", nc, ccap));
	MF_TRY(check_list("particleSurfaceTurbulence", Rc));
	kills_host[0] = kills_host[1] = kills_host[2] = 0;
	if (n == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	const Cells CC = {Rc, cstart, cids};
	const Pts coarse = {nc, ccap, cpos, cflag}, surf = {n, cap, pos, flag};
	MF_HIP(hipMemsetAsync(head, 0, 3 * sizeof(int32_t), st));
	ST_LAUNCH(k_delete, n, st, load_par(par_host), CC, coarse, surf, flag, state, head);
	MF_LAUNCH_CHECK();
	return read_back(kills_host, head, 3 * sizeof(int32_t), st);
}

int mf_surfturb_clear_new(int64_t n, int32_t* flag, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, n));
	if (n == 0) return 0;
	ST_LAUNCH(k_clear_new, n, (hipStream_t)stream, n, flag);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_surfturb_normals(const float* par_host, int Rc, const int32_t* cstart, const int32_t* cids, int64_t nc, int64_t ccap, const float* cpos,
                        const int32_t* cflag, int Rs, const int32_t* sstart, const int32_t* sids, int64_t n, int64_t cap, const float* pos,
                        const int32_t* flag, float* normals, float* tempv, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, cap));
	MF_TRY(check_set("particleSurfaceTurbulence", nc, ccap));
	MF_TRY(check_list("particleSurfaceTurbulence", Rc));
	MF_TRY(check_list("particleSurfaceTurbulence", Rs));
	if (n == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	const Par par = load_par(par_host);
	const Cells CC = {Rc, cstart, cids}, CS = {Rs, sstart, sids};
	const Pts coarse = {nc, ccap, cpos, cflag}, surf = {n, cap, pos, flag};
	ST_LAUNCH(k_normals, n, st, par, CC, coarse, CS, surf, normals);
	ST_LAUNCH(k_avg_normals, n, st, par, CS, surf, (const float*)normals, tempv);
	ST_LAUNCH(k_assign3<false>, n, st, n, cap, normals, (const float*)tempv);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_surfturb_regularize(const float* par_host, int Rs, const int32_t* sstart, const int32_t* sids, int64_t n, int64_t cap, float* pos,
                           const int32_t* flag, const float* normals, float* tempf, float* tempv, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, cap));
	MF_TRY(check_list("particleSurfaceTurbulence", Rs));
	if (n == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	const Par par = load_par(par_host);
	const Cells CS = {Rs, sstart, sids};
	const Pts surf = {n, cap, pos, flag};
	ST_LAUNCH(k_density, n, st, par, CS, surf, tempf);
	ST_LAUNCH(k_displacement, n, st, par, CS, surf, normals, (const float*)tempf, tempv);
	ST_LAUNCH(k_assign3<true>, n, st, n, cap, pos, (const float*)tempv);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_surfturb_constrain(const float* par_host, int Rc, const int32_t* cstart, const int32_t* cids, int64_t nc, int64_t ccap,
                          const float* cpos, const int32_t* cflag, int64_t n, int64_t cap, float* pos, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, cap));
	MF_TRY(check_set("particleSurfaceTurbulence", nc, ccap));
	MF_TRY(check_list("particleSurfaceTurbulence", Rc));
	if (n == 0) return 0;
	const Cells CC = {Rc, cstart, cids};
	const Pts coarse = {nc, ccap, cpos, cflag}, surf = {n, cap, pos, nullptr};
	ST_LAUNCH(k_constrain, n, (hipStream_t)stream, load_par(par_host), CC, coarse, surf, pos);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_surfturb_waves(const float* par_host, int Rs, const int32_t* sstart, const int32_t* sids, int64_t n, int64_t cap, const float* pos,
                      const int32_t* flag, const float* normals, float* H, float* DtH, float* source, float* seed, float* seedAmp,
                      float* tempf, float* tempv, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, cap));
	MF_TRY(check_list("particleSurfaceTurbulence", Rs));
	if (n == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	const Par par = load_par(par_host);
	const Cells CS = {Rs, sstart, sids};
	const Pts surf = {n, cap, pos, flag};
	ST_LAUNCH(k_add_seed, n, st, n, H, (const float*)seed);
	ST_LAUNCH(k_wave_normal, n, st, par, CS, surf, normals, (const float*)H, tempv);
	ST_LAUNCH(k_wave_laplacian, n, st, par, CS, surf, normals, (const float*)H, (const float*)tempv, tempf);
	ST_LAUNCH(k_evolve, n, st, par, n, H, DtH, (const float*)seed, (const float*)tempf);
	ST_LAUNCH(k_curvature, n, st, par, CS, surf, normals, tempf);
	ST_LAUNCH(k_smooth_curvature, n, st, par, CS, surf, (const float*)tempf, source);
	ST_LAUNCH(k_seed, n, st, par, n, source, seed, seedAmp);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_surfturb_save_prev(int64_t nc, int64_t ccap, const float* cpos, const int32_t* cflag, int64_t pcap, float* prev, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", nc, ccap < pcap ? ccap : pcap));
	if (nc == 0) return 0;
	const Pts coarse = {nc, ccap, cpos, cflag};
	ST_LAUNCH(k_save_prev, nc, (hipStream_t)stream, coarse, pcap, prev);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_surfturb_displaced_plan(int64_t n, const int32_t* flag, int32_t* mark, void* tmp, int64_t tmp_bytes, int64_t* total_host, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, n));
	*total_host = 0;
	if (n == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	ST_LAUNCH(k_live_mark, n, st, n, flag, mark);
	MF_LAUNCH_CHECK();
	return scan_total("particleSurfaceTurbulence", mark, n, tmp, tmp_bytes, total_host, st);
}

int mf_surfturb_displaced_fill(int64_t n, int64_t cap, const float* pos, const int32_t* flag, const float* normals, const float* H,
                               const int32_t* mark, int64_t ocap, float* out, int32_t* oflag, void* stream) {
	MF_TRY(check_set("particleSurfaceTurbulence", n, cap));
	if (n == 0) return 0;
	const Pts surf = {n, cap, pos, flag};
	ST_LAUNCH(k_displaced, n, (hipStream_t)stream, surf, normals, H, mark, ocap, out, oflag);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_surfturb_check_parts(int sx, int sy, int sz, int64_t n, int64_t cap, const float* pos, int32_t* head, int64_t* bad_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	MF_TRY(check_set("debugCheckParts", n, cap));
	*bad_host = -1;
	if (n == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_set_i32, dim3(1), dim3(64), 0, st, head, INT_MAX, 0, 0);
	ST_LAUNCH(k_check_parts, n, st, sx, sy, sz, n, cap, pos, head);
	MF_LAUNCH_CHECK();
	int32_t bad = INT_MAX;
	MF_TRY(read_back(&bad, head, sizeof(bad), st));
	*bad_host = bad == INT_MAX ? -1 : bad;
	return 0;
}

}  // extern "C"
