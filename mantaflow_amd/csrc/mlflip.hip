// mlflip.hip -- the array bridge and the MLFLIP data plugins (include/open/manta_hip_mlflip.h): the dtype conversions and the
// plane <-> element transpositions of the numpy copies, the feature matrix of extractFeatureVel / Phi / Geo with one thread per
// (particle, stencil point), connected-component labelling by union-find with the runs of a row resolved inside the wavefront, the
// rounds of extendRegion, markSmallRegions and simpleNumpyTest.
// Reference: plugin/numpyconvert.cpp:29-223, plugin/tfplugins.cpp:22-220.
#include "common.h"
#include "scan.h"
#include "../../include/open/manta_hip_mlflip.h"

using namespace mf;

namespace {

constexpr int PDELETE_BIT = 1 << 10;
constexpr int WAVE = 64;
constexpr int WAVES = BLOCK / WAVE;

Arena g_arena[MAX_DEVICES];

// ---- the copies -------------------------------------------------------------------------------------------------------------------
// one element per lane, both streams touched once
template <class S, class D>
__global__ void __launch_bounds__(BLOCK) k_convert(int64_t n, const S* __restrict__ src, D* __restrict__ dst) {
	const int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (q >= n) return;
	__builtin_nontemporal_store((D)__builtin_nontemporal_load(src + q), dst + q);
}

// arr[q][c] = planes[c][q]: the three plane loads are coalesced 4-byte accesses, the three adjacent stores of a lane one 12-byte
// (24-byte) access, contiguous from lane to lane
template <class A>
__global__ void __launch_bounds__(BLOCK) k_planes_to_elements(int64_t n, int64_t stride, const float* __restrict__ planes, A* __restrict__ arr) {
	const int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (q >= n) return;
	const float x = __builtin_nontemporal_load(planes + q);
	const float y = __builtin_nontemporal_load(planes + stride + q);
	const float z = __builtin_nontemporal_load(planes + 2 * stride + q);
	A* o = arr + 3 * q;
	__builtin_nontemporal_store((A)x, o);
	__builtin_nontemporal_store((A)y, o + 1);
	__builtin_nontemporal_store((A)z, o + 2);
}

template <class A>
__global__ void __launch_bounds__(BLOCK) k_elements_to_planes(int64_t n, int64_t stride, const A* __restrict__ arr, float* __restrict__ planes) {
	const int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (q >= n) return;
	const A* s = arr + 3 * q;
	const A x = __builtin_nontemporal_load(s);
	const A y = __builtin_nontemporal_load(s + 1);
	const A z = __builtin_nontemporal_load(s + 2);
	__builtin_nontemporal_store((float)x, planes + q);
	__builtin_nontemporal_store((float)y, planes + stride + q);
	__builtin_nontemporal_store((float)z, planes + 2 * stride + q);
}

template <class S, class D>
int launch_convert(int64_t n, const void* src, void* dst, hipStream_t st) {
	hipLaunchKernelGGL((k_convert<S, D>), dim3(nblk(n)), dim3(BLOCK), 0, st, n, (const S*)src, (D*)dst);
	MF_LAUNCH_CHECK();
	return 0;
}

int check_count(const char* who, int64_t n) {
	if (n < 0) return fail("%s: %lld elements", who, (long long)n);
	if ((n + BLOCK - 1) / BLOCK > (int64_t)0x7fffffff) return fail("%s: %lld elements are more than one launch covers", who, (long long)n);
	return 0;
}

// ---- the feature matrix -----------------------------------------------------------------------------------------------------------
struct Feat {
	Dim d;
	const void* grid;
	int64_t np, cap, total;      // total = np * nst threads
	const float* pos;
	const int32_t* pflag;
	const int32_t* ptype;
	int exclude, window, W, Wk, nst, D;
	float scale;
	float* fv;
	int64_t N_row, off_begin;
};

// KIND 0 velocity, 1 phi, 2 geo (tfplugins.cpp:38-120).  Thread t is stencil point t % nst of particle t / nst: the stores of a row are
// contiguous over the lanes and neighbouring lanes interpolate in neighbouring cells
template <int KIND>
__global__ void __launch_bounds__(BLOCK) k_extract_feature(Feat a) {
	const int64_t t = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (t >= a.total) return;
	const int64_t p = t / a.nst;
	const int s = (int)(t - p * a.nst);
	if (a.pflag[p] & PDELETE_BIT) return;
	if (a.ptype && (a.ptype[p] & a.exclude)) return;
	const int kq = s % a.Wk;
	const int r = s / a.Wk;
	const int jq = r % a.W, iq = r / a.W;
	const float x = a.pos[p] + (float)(iq - a.window);
	const float y = a.pos[a.cap + p] + (float)(jq - a.window);
	float z = a.pos[2 * a.cap + p] + (float)(a.d.is3d ? kq - a.window : 0);
	if (!a.d.is3d && !(z < 1.f)) z = 0.5f;      // a 2-D grid has the one plane: no z position may index a second one
	float* o = a.fv + (p * a.N_row + a.off_begin + (int64_t)s * a.D);
	if (KIND == 0) {
		float vx, vy, vz;
		interpol_mac(a.d, (const float*)a.grid, x, y, z, vx, vy, vz);
		o[0] = vx * a.scale;
		o[1] = vy * a.scale;
		if (a.d.is3d) o[2] = vz * a.scale;
	} else if (KIND == 1) {
		o[0] = interpol1(a.d, (const float*)a.grid, x, y, z) * a.scale;
	} else {
		// FlagGrid::getAt(Vec3), grid.h:323: the cell the position truncates to.  The reference indexes unchecked; here the cell is
		// clamped into the grid, which changes nothing for a position inside (the plugin's precondition)
		int ci = (int)x, cj = (int)y, ck = (int)z;
		ci = ci < 0 ? 0 : (ci > a.d.sx - 1 ? a.d.sx - 1 : ci);
		cj = cj < 0 ? 0 : (cj > a.d.sy - 1 ? a.d.sy - 1 : cj);
		ck = ck < 0 ? 0 : (ck > a.d.sz - 1 ? a.d.sz - 1 : ck);
		const int32_t f = ((const int32_t*)a.grid)[(int64_t)ci + a.d.Y * cj + a.d.Z * ck];
		o[0] = (float)f * a.scale;
	}
}

// ---- regions ----------------------------------------------------------------------------------------------------------------------
// One wavefront per segment of 64 cells of a row, lanes along x.  `act` is the ballot of the segment's ctype cells; a run is a maximal
// group of set bits, so the cells of a run are connected along x without touching memory.
struct Seg {
	Dim d;
	int segs;          // segments per row
	int64_t waves;     // rows * segs
};

struct Lane {
	bool in;           // the wavefront has a segment
	int i, lane;
	int64_t idx, base; // this cell, lane 0 of the segment
	int64_t row;       // j + sy * k
};

__device__ __forceinline__ Lane seg_lane(const Seg& g) {
	Lane L;
	const int64_t w = blockIdx.x * (int64_t)WAVES + (threadIdx.x >> 6);
	L.lane = threadIdx.x & 63;
	L.in = w < g.waves;
	const int64_t row = w / g.segs;
	const int seg = (int)(w - row * g.segs);
	L.row = row;
	L.i = seg * WAVE + L.lane;
	L.base = row * g.d.sx + (int64_t)seg * WAVE;
	L.idx = L.base + L.lane;
	return L;
}
// first lane of the run that bit `lane` of `act` belongs to
__device__ __forceinline__ int run_start(unsigned long long act, int lane) {
	const unsigned long long gaps = ~act & ((1ull << lane) - 1ull);
	return gaps ? 64 - __clzll((long long)gaps) : 0;
}
// cells of the run that starts at bit `start`
__device__ __forceinline__ int run_length(unsigned long long act, int start) {
	const unsigned long long rest = ~act >> start;
	return rest ? __ffsll((long long)rest) - 1 : 64 - start;
}
// first lane of a maximal group of set bits?
__device__ __forceinline__ bool group_head(unsigned long long m, int lane) {
	return ((m >> lane) & 1ull) && (lane == 0 || !((m >> (lane - 1)) & 1ull));
}

__device__ __forceinline__ int32_t uf_load(const int32_t* parent, int32_t x) {
	return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// parents only ever decrease and stay inside the component, so a stale value is a longer way to the same root
__device__ __forceinline__ int32_t uf_find(const int32_t* parent, int32_t x) {
	for (;;) {
		const int32_t p = uf_load(parent, x);
		if (p == x) return x;
		x = p;
	}
}
// hang the larger root under the smaller one; where another thread got there first the atomic says so and the union goes on from what
// it found.  Lock-free: a retry means another union succeeded, and no thread waits for another
__device__ __forceinline__ void uf_unite(int32_t* parent, int32_t a, int32_t b) {
	for (;;) {
		a = uf_find(parent, a);
		b = uf_find(parent, b);
		if (a == b) return;
		if (a < b) {
			const int32_t h = a;
			a = b;
			b = h;
		}
		const int32_t old = atomicMin(parent + a, b);
		if (old == a) return;
		a = old;
	}
}

// parent = the first cell of the run inside the segment, -1 outside ctype
__global__ void __launch_bounds__(BLOCK) k_region_init(Seg g, const int32_t* __restrict__ flags, int ctype, int32_t* __restrict__ parent) {
	const Lane L = seg_lane(g);
	const bool cell = L.in && L.i < g.d.sx;
	const bool on = cell && (flags[L.idx] & ctype);
	const unsigned long long act = __ballot(on);
	if (cell) parent[L.idx] = on ? (int32_t)(L.base + run_start(act, L.lane)) : -1;
}

// the unions across the seam of two segments and with the rows at -y and -z: one per maximal group of cells that face a ctype cell of
// that row, by the group's first lane
__global__ void __launch_bounds__(BLOCK) k_region_union(Seg g, const int32_t* __restrict__ flags, int ctype, int32_t* __restrict__ parent) {
	const Lane L = seg_lane(g);
	const Dim& d = g.d;
	const bool cell = L.in && L.i < d.sx;
	const bool on = cell && (flags[L.idx] & ctype);
	const int j = (int)(L.row % d.sy), k = (int)(L.row / d.sy);
	const bool ony = on && j > 0 && (flags[L.idx - d.sx] & ctype);
	const bool onz = on && k > 0 && (flags[L.idx - (int64_t)d.sx * d.sy] & ctype);
	const unsigned long long my = __ballot(ony), mz = __ballot(onz);
	if (!on) return;
	if (L.lane == 0 && L.i > 0 && (flags[L.idx - 1] & ctype)) uf_unite(parent, (int32_t)L.idx, (int32_t)(L.idx - 1));
	if (group_head(my, L.lane)) uf_unite(parent, (int32_t)L.idx, (int32_t)(L.idx - d.sx));
	if (group_head(mz, L.lane)) uf_unite(parent, (int32_t)L.idx, (int32_t)(L.idx - (int64_t)d.sx * d.sy));
}

// parent = the root.  MARK: mark[idx] = 1 at the roots (mark[n] = 0 closes the scan).  COUNT: the first lane of every run adds the run's
// length to the root's counter
template <bool COUNT>
__global__ void __launch_bounds__(BLOCK) k_region_flatten(Seg g, int32_t* __restrict__ parent, int32_t* __restrict__ aux) {
	const Lane L = seg_lane(g);
	const bool cell = L.in && L.i < g.d.sx;
	int32_t root = -1;
	if (cell && uf_load(parent, (int32_t)L.idx) >= 0) root = uf_find(parent, (int32_t)L.idx);
	const unsigned long long act = __ballot(root >= 0);
	if (!cell) return;
	if (root >= 0) parent[L.idx] = root;
	if (COUNT) {
		if (group_head(act, L.lane)) atomicAdd(aux + root, run_length(act, L.lane));
	} else {
		aux[L.idx] = root == (int32_t)L.idx ? 1 : 0;
		if (L.idx == g.d.n - 1) aux[g.d.n] = 0;
	}
}

// r = the value at the root (+ 1: the number of roots before it, plus one), 0 outside
__global__ void __launch_bounds__(BLOCK) k_region_gather(int64_t n, const int32_t* __restrict__ parent, const int32_t* __restrict__ aux, int add, int32_t* __restrict__ r) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	const int32_t root = parent[idx];
	r[idx] = root >= 0 ? aux[root] + add : 0;
}

// one round of extendRegion, tfplugins.cpp:190-207
__global__ void __launch_bounds__(BLOCK) k_extend_region(Dim d, const int32_t* __restrict__ src, int32_t* __restrict__ dst, int region, int exclude) {
	CELL_IJK(d)
	const int32_t f = src[idx];
	bool hit = false;
	if (!(f & exclude)) {
		hit = (i > 0 && (src[idx - 1] & region)) || (i < d.sx - 1 && (src[idx + 1] & region)) || (j > 0 && (src[idx - d.sx] & region)) ||
		      (j < d.sy - 1 && (src[idx + d.sx] & region));
		if (!hit && d.is3d) hit = (k > 0 && (src[idx - d.Z] & region)) || (k < d.sz - 1 && (src[idx + d.Z] & region));
	}
	dst[idx] = hit ? region : f;
}

__global__ void __launch_bounds__(BLOCK) k_mark_small_regions(int64_t n, int32_t* __restrict__ flags, const int32_t* __restrict__ rcnt, int mark, int exclude, int th) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	if (flags[idx] & exclude) return;
	if (rcnt[idx] <= th) flags[idx] = mark;
}

// knSimpleNumpyTest, tfplugins.cpp:22-27
__global__ void __launch_bounds__(BLOCK) k_simple_array_add(Dim d, float* __restrict__ grid, const float* __restrict__ arr, float scale) {
	CELL_IJK(d)
	grid[idx] += scale * arr[(int64_t)j * d.sx + i];
}

int whole_domain(const char* who, int sx, int sy, int sz) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("%s: not available inside a z-slab window", who);
	return 0;
}

}  // namespace

extern "C" {

int mf_mlflip_abi_version(void) { return MF_MLFLIP_ABI_VERSION; }

int mf_mlflip_convert(int64_t n, const void* src, int src_type, void* dst, int dst_type, void* stream) {
	MF_TRY(check_count("mf_mlflip_convert", n));
	if (src_type < 0 || src_type > 2 || dst_type < 0 || dst_type > 2) return fail("mf_mlflip_convert: element types %d -> %d", src_type, dst_type);
	if (n == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	if (src_type == dst_type) {
		MF_HIP(hipMemcpyAsync(dst, src, (size_t)n * (src_type == MF_MLFLIP_FLOAT64 ? 8 : 4), hipMemcpyDeviceToDevice, st));
		return 0;
	}
	switch (src_type * 3 + dst_type) {
	case 0 * 3 + 1: return launch_convert<int32_t, float>(n, src, dst, st);
	case 0 * 3 + 2: return launch_convert<int32_t, double>(n, src, dst, st);
	case 1 * 3 + 0: return launch_convert<float, int32_t>(n, src, dst, st);
	case 1 * 3 + 2: return launch_convert<float, double>(n, src, dst, st);
	case 2 * 3 + 0: return launch_convert<double, int32_t>(n, src, dst, st);
	default: return launch_convert<double, float>(n, src, dst, st);
	}
}

int mf_mlflip_planes_to_elements(int64_t n, int64_t stride, const float* planes, void* arr, int arr_type, void* stream) {
	MF_TRY(check_count("mf_mlflip_planes_to_elements", n));
	if (stride < n) return fail("mf_mlflip_planes_to_elements: %lld elements in planes of stride %lld", (long long)n, (long long)stride);
	if (arr_type != MF_MLFLIP_FLOAT32 && arr_type != MF_MLFLIP_FLOAT64) return fail("unknown/unsupported type of Vec3 Numpy array");
	if (n == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	if (arr_type == MF_MLFLIP_FLOAT32) hipLaunchKernelGGL(k_planes_to_elements<float>, dim3(nblk(n)), dim3(BLOCK), 0, st, n, stride, planes, (float*)arr);
	else hipLaunchKernelGGL(k_planes_to_elements<double>, dim3(nblk(n)), dim3(BLOCK), 0, st, n, stride, planes, (double*)arr);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mlflip_elements_to_planes(int64_t n, int64_t stride, const void* arr, int arr_type, float* planes, void* stream) {
	MF_TRY(check_count("mf_mlflip_elements_to_planes", n));
	if (stride < n) return fail("mf_mlflip_elements_to_planes: %lld elements in planes of stride %lld", (long long)n, (long long)stride);
	if (arr_type != MF_MLFLIP_FLOAT32 && arr_type != MF_MLFLIP_FLOAT64) return fail("unknown/unsupported type of Vec3 Numpy array");
	if (n == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	if (arr_type == MF_MLFLIP_FLOAT32) hipLaunchKernelGGL(k_elements_to_planes<float>, dim3(nblk(n)), dim3(BLOCK), 0, st, n, stride, (const float*)arr, planes);
	else hipLaunchKernelGGL(k_elements_to_planes<double>, dim3(nblk(n)), dim3(BLOCK), 0, st, n, stride, (const double*)arr, planes);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mlflip_extract_feature(int kind, int sx, int sy, int sz, const void* grid, int64_t np, int64_t cap, const float* pos,
                              const int32_t* pflag, const int32_t* ptype, int exclude, int window, float scale, float* fv, int64_t fv_len,
                              int64_t N_row, int64_t off_begin, void* stream) {
	static const char* const names[3] = {"extractFeatureVel", "extractFeaturePhi", "extractFeatureGeo"};
	if (kind < 0 || kind > 2) return fail("mf_mlflip_extract_feature: kind %d", kind);
	const char* who = names[kind];
	MF_TRY(whole_domain(who, sx, sy, sz));
	if (np < 0 || cap < np) return fail("%s: %lld particles in arrays of stride %lld", who, (long long)np, (long long)cap);
	if (window < 0 || window > 64) return fail("%s: window %d", who, window);
	const Dim d = mkdim(sx, sy, sz);
	const int W = 2 * window + 1, Wk = d.is3d ? W : 1;
	const int nst = W * W * Wk, D = kind == 0 ? (d.is3d ? 3 : 2) : 1;
	if (off_begin < 0 || N_row < 0 || off_begin + (int64_t)nst * D > N_row)
		return fail("%s: %d stencil points of %d values from column %lld do not fit a row of %lld", who, nst, D, (long long)off_begin, (long long)N_row);
	if (N_row > 0 && np > (((int64_t)1 << 62) / N_row)) return fail("%s: %lld rows of %lld", who, (long long)np, (long long)N_row);
	if (fv_len < np * N_row) return fail("%s: the feature array holds %lld values, %lld rows of %lld need %lld", who, (long long)fv_len, (long long)np, (long long)N_row, (long long)(np * N_row));
	if (np == 0) return 0;
	if (np > (((int64_t)1 << 38) / nst)) return fail("%s: %lld particles of %d stencil points are more than one launch covers", who, (long long)np, nst);
	Feat a;
	a.d = d;
	a.grid = grid;
	a.np = np;
	a.cap = cap;
	a.total = np * nst;
	a.pos = pos;
	a.pflag = pflag;
	a.ptype = ptype;
	a.exclude = exclude;
	a.window = window;
	a.W = W;
	a.Wk = Wk;
	a.nst = nst;
	a.D = D;
	a.scale = scale;
	a.fv = fv;
	a.N_row = N_row;
	a.off_begin = off_begin;
	const hipStream_t st = (hipStream_t)stream;
	const dim3 grd(nblk(a.total));
	if (kind == 0) hipLaunchKernelGGL(k_extract_feature<0>, grd, dim3(BLOCK), 0, st, a);
	else if (kind == 1) hipLaunchKernelGGL(k_extract_feature<1>, grd, dim3(BLOCK), 0, st, a);
	else hipLaunchKernelGGL(k_extract_feature<2>, grd, dim3(BLOCK), 0, st, a);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mlflip_regions(int sx, int sy, int sz, const int32_t* flags, int ctype, int counts, int32_t* r, int32_t* count_host, void* stream) {
	const char* who = counts ? "getRegionalCounts" : "getRegions";
	MF_TRY(whole_domain(who, sx, sy, sz));
	const hipStream_t st = (hipStream_t)stream;
	Seg g;
	g.d = mkdim(sx, sy, sz);
	g.segs = (sx + WAVE - 1) / WAVE;
	g.waves = (int64_t)sy * sz * g.segs;
	const int64_t n = g.d.n;
	size_t ws_bytes = 0;
	if (!counts) MF_TRY(exclusive_sum32_bytes(n + 1, &ws_bytes));
	const size_t need = 2 * al256(sizeof(int32_t) * (size_t)(n + 1)) + al256(ws_bytes) + 256;
	Arena* a;
	MF_TRY(arena_reserve(g_arena, need, &a));
	Cutter c(a->p, need);
	int32_t *parent, *aux;
	char* ws;
	MF_TRY(c.take((size_t)n + 1, &parent, &aux));
	MF_TRY(c.take(ws_bytes + 1, &ws));
	const dim3 seg_grid((unsigned)((g.waves + WAVES - 1) / WAVES));
	hipLaunchKernelGGL(k_region_init, seg_grid, dim3(BLOCK), 0, st, g, flags, ctype, parent);
	hipLaunchKernelGGL(k_region_union, seg_grid, dim3(BLOCK), 0, st, g, flags, ctype, parent);
	MF_LAUNCH_CHECK();
	if (counts) {
		MF_HIP(hipMemsetAsync(aux, 0, sizeof(int32_t) * (size_t)n, st));
		hipLaunchKernelGGL(k_region_flatten<true>, seg_grid, dim3(BLOCK), 0, st, g, parent, aux);
		hipLaunchKernelGGL(k_region_gather, dim3(nblk(n)), dim3(BLOCK), 0, st, n, parent, aux, 0, r);
		MF_LAUNCH_CHECK();
		return 0;
	}
	hipLaunchKernelGGL(k_region_flatten<false>, seg_grid, dim3(BLOCK), 0, st, g, parent, aux);
	MF_LAUNCH_CHECK();
	MF_TRY(exclusive_sum(ws, ws_bytes, aux, aux, n + 1, st));      // aux[idx] = the roots before idx, aux[n] = all of them
	hipLaunchKernelGGL(k_region_gather, dim3(nblk(n)), dim3(BLOCK), 0, st, n, parent, aux, 1, r);
	MF_LAUNCH_CHECK();
	Workspace* w;
	MF_TRY(get_workspace(&w));
	return read_scalars(w, aux + n, sizeof(int32_t), count_host, st);
}

int mf_mlflip_extend_region(int sx, int sy, int sz, int32_t* flags, int32_t* tmp, int region, int exclude, int depth, void* stream) {
	MF_TRY(whole_domain("extendRegion", sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	const hipStream_t st = (hipStream_t)stream;
	int32_t* src = flags;
	int32_t* dst = tmp;
	for (int q = 0; q < depth; q++) {
		hipLaunchKernelGGL(k_extend_region, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, src, dst, region, exclude);
		MF_LAUNCH_CHECK();
		int32_t* h = src;
		src = dst;
		dst = h;
	}
	if (src != flags) MF_HIP(hipMemcpyAsync(flags, tmp, sizeof(int32_t) * (size_t)d.n, hipMemcpyDeviceToDevice, st));      // an odd number of rounds
	return 0;
}

int mf_mlflip_mark_small_regions(int sx, int sy, int sz, int32_t* flags, const int32_t* rcnt, int mark, int exclude, int th, void* stream) {
	MF_TRY(whole_domain("markSmallRegions", sx, sy, sz));
	const int64_t n = (int64_t)sx * sy * sz;
	hipLaunchKernelGGL(k_mark_small_regions, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, flags, rcnt, mark, exclude, th);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mlflip_simple_array_add(int sx, int sy, int sz, float* grid, const float* arr, int64_t arr_len, float scale, void* stream) {
	MF_TRY(whole_domain("simpleNumpyTest", sx, sy, sz));
	if (arr_len < (int64_t)sx * sy) return fail("simpleNumpyTest: the array holds %lld values, a plane of the grid has %lld", (long long)arr_len, (long long)sx * sy);
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_simple_array_add, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, grid, arr, scale);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
