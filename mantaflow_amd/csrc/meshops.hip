// meshops.hip -- mesh connectivity and smoothing (include/open/manta_hip_meshops.h): the corner table and the 1-ring lookup from stable
// radix sorts of the corners (two 32-bit passes per 64-bit key), smoothMesh as one lane per node walking its ring in ascending order,
// and computeCenterOfMass as per-triangle fp64 terms summed in a fixed tree.  The per-element bodies are in meshops_cells.h.
// Reference: mesh.cpp:123-141, 238-292, plugin/meshplugins.cpp:36-104.
#include "meshops_cells.h"
#include "reduce.h"
#include "../../include/open/manta_hip_meshops.h"
#include "scan.h"
#include <limits.h>

using namespace mf;
using namespace mf::meshops;

namespace {

// the head of the scratch as ints: [0] groups of one, [1] groups of three or more, [2] the first triangle with a repeated node,
// [3] the first triangle that names a node outside the mesh (INT_MAX: none)
__global__ void k_head_init(int32_t* __restrict__ head) {
	if (blockIdx.x || threadIdx.x) return;
	head[0] = head[1] = 0;
	head[2] = head[3] = INT_MAX;
}
__device__ __forceinline__ bool refused(const int32_t* __restrict__ head) { return head[2] != INT_MAX || head[3] != INT_MAX; }

__global__ void __launch_bounds__(BLOCK) k_validate(Tris T, int32_t* __restrict__ head) {
	const int64_t t = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (t >= T.nTris) return;
	const int f = tri_fault(T, t);
	if (f) atomicMin(&head[f == 2 ? 2 : 3], (int32_t)t);
}

// which 0: the larger node of the corner's edge, 1: the corner's own node; the value is the corner
__global__ void __launch_bounds__(BLOCK) k_corner_keys(Tris T, int which, uint32_t* __restrict__ key, int32_t* __restrict__ val) {
	const int64_t c = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (c >= 3 * T.nTris) return;
	int32_t lo, hi;
	edge_key(T, c, lo, hi);
	key[c] = (uint32_t)(which ? corner_node(T, c) : hi);
	val[c] = (int32_t)c;
}
__global__ void __launch_bounds__(BLOCK) k_corner_lo(Tris T, const int32_t* __restrict__ head, const int32_t* __restrict__ val, uint32_t* __restrict__ key) {
	const int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (s >= 3 * T.nTris) return;
	int32_t lo = 0, hi;
	if (!refused(head)) edge_key(T, val[s], lo, hi);
	key[s] = (uint32_t)lo;
}
__global__ void __launch_bounds__(BLOCK) k_groups(Tris T, const int32_t* __restrict__ sorted, int32_t* __restrict__ opposite, int32_t* __restrict__ head) {
	const int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (s >= 3 * T.nTris || refused(head)) return;
	const int r = group_entry(T, 3 * T.nTris, sorted, s, opposite);
	if (r & 1) atomicAdd(&head[0], 1);
	if (r & 2) atomicAdd(&head[1], 1);
}
// corners sorted by node (ascending corner, so ascending triangle, within a node): the triangles of the 1-ring
__global__ void __launch_bounds__(BLOCK)
k_tri_csr(Tris T, const int32_t* __restrict__ head, const uint32_t* __restrict__ node, const int32_t* __restrict__ sorted, int32_t* __restrict__ triOff,
          int32_t* __restrict__ ringTris) {
	const int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	const int64_t m = 3 * T.nTris;
	if (s >= m || refused(head)) return;
	ringTris[s] = sorted[s] / 3;
	csr_offsets(triOff, T.nNodes, s, m, s ? (int32_t)node[s - 1] : -1, (int32_t)node[s], (int32_t)s, (int32_t)m);
}

__global__ void __launch_bounds__(BLOCK) k_pair_keys(Tris T, uint32_t* __restrict__ key, int32_t* __restrict__ val) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= 6 * T.nTris) return;
	key[p] = (uint32_t)pair_neighbour(T, p);
	val[p] = (int32_t)p;
}
__global__ void __launch_bounds__(BLOCK) k_pair_node(Tris T, const int32_t* __restrict__ head, const int32_t* __restrict__ val, uint32_t* __restrict__ key) {
	const int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (s >= 6 * T.nTris) return;
	key[s] = refused(head) ? 0u : (uint32_t)pair_node(T, val[s]);
}
__global__ void __launch_bounds__(BLOCK) k_pair_first(Tris T, const int32_t* __restrict__ head, const int32_t* __restrict__ sorted, int32_t* __restrict__ first) {
	const int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (s >= 6 * T.nTris) return;
	first[s] = refused(head) ? 0 : pair_is_first(T, sorted, s);
}
__global__ void __launch_bounds__(BLOCK)
k_ring_csr(Tris T, const int32_t* __restrict__ head, const uint32_t* __restrict__ node, const int32_t* __restrict__ sorted, const int32_t* __restrict__ rank,
           int32_t* __restrict__ nodeOff, int32_t* __restrict__ ringNodes) {
	const int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	const int64_t m = 6 * T.nTris;
	if (s >= m || refused(head)) return;
	const int32_t first = pair_is_first(T, sorted, s), r = rank[s];
	if (first) ringNodes[r] = pair_neighbour(T, sorted[s]);
	csr_offsets(nodeOff, T.nNodes, s, m, s ? (int32_t)node[s - 1] : -1, (int32_t)node[s], r, r + first);
}

__global__ void __launch_bounds__(BLOCK)
k_smooth(Nodes N, const int32_t* __restrict__ nodeOff, const int32_t* __restrict__ ringNodes, const int32_t* __restrict__ triOff, float str, float minLength,
         float* __restrict__ temp) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= N.n) return;
	float out[3];
	smooth_node(N, nodeOff, ringNodes, triOff, p, str, minLength, out);
	for (int c = 0; c < 3; c++) temp[c * N.n + p] = out[c];
}
__global__ void __launch_bounds__(BLOCK) k_copy_back(int64_t n, int64_t ncap, float* __restrict__ pos, const int32_t* __restrict__ flags, const float* __restrict__ temp) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= n || (flags[p] & 1)) return;     // Mesh::NfFixed
	for (int c = 0; c < 3; c++) pos[c * ncap + p] = temp[c * n + p];
}

__global__ void __launch_bounds__(BLOCK) k_volume_terms(Tris T, int64_t ncap, const float* __restrict__ pos, double* __restrict__ terms) {
	const int64_t t = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (t >= T.nTris) return;
	double v[4];
	volume_terms(T, ncap, pos, t, v);
	for (int q = 0; q < 4; q++) terms[q * T.nTris + t] = v[q];
}
// the four sums of the triangles' terms, one triangle per thread, in the fixed tree of reduce.h
struct VolumeTerm {
	Tris T;
	int64_t ncap;
	const float* pos;
	__device__ __forceinline__ void operator()(int64_t t, double (&acc)[4]) const {
		double v[4];
		volume_terms(T, ncap, pos, t, v);
		for (int q = 0; q < 4; q++) acc[q] += v[q];
	}
};

__global__ void __launch_bounds__(BLOCK)
k_rescale(int64_t n, int64_t ncap, float* __restrict__ pos, const int32_t* __restrict__ flags, float ox, float oy, float oz, float nx, float ny, float nz,
          float beta) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= n || (flags[p] & 1)) return;
	const float o[3] = {ox, oy, oz}, m[3] = {nx, ny, nz};
	for (int c = 0; c < 3; c++) pos[c * ncap + p] = rescale_component(pos[c * ncap + p], o[c], m[c], beta);
}

int check_sizes(const char* who, int64_t nTris, int64_t tcap, int64_t nNodes, int64_t ncap) {
	if (nTris < 0 || tcap < nTris || nNodes < 0 || ncap < nNodes)
		return fail("%s: %lld triangles / %lld nodes in arrays of stride %lld / %lld", who, (long long)nTris, (long long)nNodes, (long long)tcap, (long long)ncap);
	if (6 * nTris >= (int64_t)1 << 31 || nNodes >= ((int64_t)1 << 31) - 1) return fail("%s: too many triangles or nodes for 32-bit corner numbers", who);
	if (g_slab_gsz > 0) return fail("%s: not available inside a z-slab window", who);
	return 0;
}
// behind the head: four rows of 6 * nTris ints (keys and values, in and out), then the larger of the sort's and the scan's workspace;
// the partials of the volume sums (4 doubles per block of triangles) fit the rows.  The errors of the queries (no device) are passed
// over: the entries that use the scratch fail at their first launch there
int64_t tmp_need(int64_t nTris, int64_t nNodes) {
	const int64_t m = 6 * nTris;
	size_t b = 0;
	if (m > 0) {
		(void)sort_pairs_bytes(m, key_bits(nNodes), &b);
		(void)exclusive_sum32_bytes(m, &b);
	}
	return head_ws_bytes(4 * al256(sizeof(int32_t) * (size_t)(m > 0 ? m : 1)) + b);
}

// ---- killSmallComponents ----
// the head of the scratch as ints: [0] a label changed in this round, [1] tainted triangles, [2] deleted nodes, [3] the smallest deleted
// node that a kept triangle names (INT_MAX: none), [4] components
__global__ void __launch_bounds__(BLOCK) k_fill_i32(int64_t n, int32_t* __restrict__ a, int32_t v, int iota) {
	const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (i < n) a[i] = iota ? (int32_t)i : v;
}
__device__ __forceinline__ int32_t label_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// hook: a triangle that sees a smaller label across an edge gives it to its own root and to itself.  A label is always the number of a
// triangle of the same component, and only ever decreases
__global__ void __launch_bounds__(BLOCK) k_hook(int64_t nTris, const int32_t* __restrict__ opposite, int32_t* __restrict__ label, int32_t* __restrict__ head) {
	const int64_t t = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (t >= nTris) return;
	const int32_t lt = label_load(&label[t]);
	int32_t m = lt;
	for (int c = 0; c < 3; c++) {
		const int32_t op = opposite[3 * t + c];
		if (op < 0 || op >= 3 * nTris) continue;
		const int32_t l = label_load(&label[op / 3]);
		m = l < m ? l : m;
	}
	if (m < lt) {
		atomicMin(&label[lt], m);
		atomicMin(&label[t], m);
		head[0] = 1;
	}
}
// pointer jumping to the root (label[r] == r); a root does not change during this launch
__global__ void __launch_bounds__(BLOCK) k_jump(int64_t nTris, int32_t* __restrict__ label) {
	const int64_t t = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (t >= nTris) return;
	int32_t l = label_load(&label[t]);
	for (;;) {
		const int32_t ll = label_load(&label[l]);
		if (ll == l) break;
		l = ll;
	}
	label[t] = l;
}
__global__ void __launch_bounds__(BLOCK) k_comp_sizes(int64_t nTris, const int32_t* __restrict__ label, int32_t* __restrict__ size, int32_t* __restrict__ head) {
	const int64_t t = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	const bool active = t < nTris;
	const int32_t l = active ? label[t] : -1;
	// a surface is mostly one component: the lanes that share the label of the wave's first lane add their count with one atomic
	// (block b starts at triangle 256 b, so the first lane of every wave is active when any lane is)
	const int32_t l0 = __shfl(l, 0, 64);
	const unsigned long long same = __ballot(active && l == l0);
	if (!active) return;
	if (l != l0)
		atomicAdd(&size[l], 1);
	else if ((threadIdx.x & 63) == 0)
		atomicAdd(&size[l0], (int32_t)__popcll(same));
	if (l == (int32_t)t) atomicAdd(&head[4], 1);
}
__global__ void __launch_bounds__(BLOCK)
k_taint(int64_t nTris, const int32_t* __restrict__ label, const int32_t* __restrict__ size, int elements, int32_t* __restrict__ taint, int32_t* __restrict__ head) {
	const int64_t t = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (t >= nTris) return;
	const int32_t x = size[label[t]] < elements ? 1 : 0;
	taint[t] = x;
	if (x) atomicAdd(&head[1], 1);
}
__global__ void __launch_bounds__(BLOCK) k_first_corner(Tris T, const int32_t* __restrict__ taint, int32_t* __restrict__ first) {
	const int64_t c = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (c >= 3 * T.nTris || !taint[c / 3]) return;
	atomicMin(&first[corner_node(T, c)], (int32_t)c);
}
__global__ void __launch_bounds__(BLOCK)
k_shared_and_flags(Tris T, const int32_t* __restrict__ taint, const int32_t* __restrict__ first, int32_t* __restrict__ cflag, int32_t* __restrict__ head) {
	const int64_t c = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (c >= 3 * T.nTris) return;
	cflag[c] = is_first_tainted_corner(T, taint, first, c);
	const int32_t v = corner_node(T, c);
	if (!taint[c / 3] && first[v] != INT_MAX) atomicMin(&head[3], v);
}
__global__ void __launch_bounds__(BLOCK)
k_deleted_list(Tris T, const int32_t* __restrict__ taint, const int32_t* __restrict__ first, const int32_t* __restrict__ crank, int32_t* __restrict__ deleted,
               int32_t* __restrict__ head) {
	const int64_t c = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (c >= 3 * T.nTris) return;
	const int32_t f = is_first_tainted_corner(T, taint, first, c);
	if (f) deleted[crank[c]] = corner_node(T, c);
	if (c == 3 * T.nTris - 1) head[2] = crank[c] + f;
}
__global__ void __launch_bounds__(BLOCK)
k_fill_holes(int64_t nTris, int64_t tcap, int32_t K, const int32_t* __restrict__ taint, const int32_t* __restrict__ below, int32_t* __restrict__ tri,
             int32_t* __restrict__ tflags) {
	const int64_t h = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (h >= nTris - K || !taint[h]) return;
	const int64_t q = hole_source(taint, below, nTris, K, h);     // q >= nTris - K: no lane writes what another reads
	for (int c = 0; c < 3; c++) tri[c * tcap + h] = tri[c * tcap + q];
	tflags[h] = tflags[q];
}
__global__ void __launch_bounds__(BLOCK)
k_node_flags(int64_t D, int64_t newsize, const int32_t* __restrict__ deleted, const int32_t* __restrict__ first, int32_t* __restrict__ spotFlag,
             int32_t* __restrict__ keptFlag) {
	const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (i >= D) return;
	spotFlag[i] = deleted[i] < newsize ? 1 : 0;
	keptFlag[i] = first[newsize + i] == INT_MAX ? 1 : 0;
}
__global__ void __launch_bounds__(BLOCK)
k_spots(int64_t D, const int32_t* __restrict__ deleted, const int32_t* __restrict__ spotFlag, const int32_t* __restrict__ spotRank, int32_t* __restrict__ spot) {
	const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (i < D && spotFlag[i]) spot[spotRank[i]] = deleted[i];
}
// node newsize + i moves to newIndex[i] with its position, normal and flags; sources are >= newsize and targets below it
__global__ void __launch_bounds__(BLOCK)
k_move_nodes(int64_t D, int64_t newsize, int64_t ncap, const int32_t* __restrict__ keptFlag, const int32_t* __restrict__ keptRank,
             const int32_t* __restrict__ spot, int32_t* __restrict__ newIndex, float* __restrict__ pos, float* __restrict__ normal, int32_t* __restrict__ nflags) {
	const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (i >= D) return;
	const int32_t j = node_new_index(keptFlag, keptRank, spot, i);
	newIndex[i] = j;
	if (j < 0) return;
	for (int c = 0; c < 3; c++) {
		pos[c * ncap + j] = pos[c * ncap + newsize + i];
		normal[c * ncap + j] = normal[c * ncap + newsize + i];
	}
	nflags[j] = nflags[newsize + i];
}
__global__ void __launch_bounds__(BLOCK)
k_remap_tris(int64_t nTris, int64_t tcap, int64_t newsize, int64_t D, const int32_t* __restrict__ newIndex, int32_t* __restrict__ tri) {
	const int64_t e = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (e >= 3 * nTris) return;
	int32_t* p = &tri[(e / nTris) * tcap + e % nTris];
	const int64_t v = *p;
	if (v >= newsize && v < newsize + D) *p = newIndex[v - newsize];
}

struct KillWs {
	int32_t *head, *label, *size, *taint, *below, *first, *cflag, *deleted, *spotFlag, *keptFlag, *spotRank, *keptRank, *spot, *newIndex;
	void* ws;
	size_t ws_bytes;
};
int64_t kill_need(int64_t nTris, int64_t nNodes) {
	const size_t t = al256(sizeof(int32_t) * (size_t)(nTris > 0 ? nTris : 1)), n = al256(sizeof(int32_t) * (size_t)(nNodes > 0 ? nNodes : 1));
	size_t b = 0;
	if (nTris > 0) (void)exclusive_sum32_bytes(3 * nTris, &b);
	if (nNodes > 0) (void)exclusive_sum32_bytes(nNodes, &b);
	return head_ws_bytes(4 * t + al256(3 * t) + 8 * n + b);
}
int kill_cut(void* tmp, int64_t tmp_bytes, int64_t nTris, int64_t nNodes, KillWs* w) {
	HeadWs t;
	MF_TRY(head_ws_cut("killSmallComponents", tmp, tmp_bytes, kill_need(nTris, nNodes), &t));
	w->head = (int32_t*)t.head;
	Cutter cut(t.ws, t.ws_bytes);
	const size_t nt = (size_t)(nTris > 0 ? nTris : 1), nn = (size_t)(nNodes > 0 ? nNodes : 1);
	MF_TRY(cut.take(nt, &w->label, &w->size, &w->taint, &w->below));
	MF_TRY(cut.take(3 * nt, &w->cflag));
	MF_TRY(cut.take(nn, &w->first, &w->deleted, &w->spotFlag, &w->keptFlag, &w->spotRank, &w->keptRank, &w->spot, &w->newIndex));
	w->ws = cut.p;
	w->ws_bytes = cut.left;
	return 0;
}

}  // namespace

extern "C" {

int mf_meshops_abi_version(void) { return MF_MESHOPS_ABI_VERSION; }

int mf_meshops_tmp_bytes(int64_t nTris, int64_t nNodes, int64_t* bytes_host) {
	if (nTris < 0 || nNodes < 0 || 6 * nTris >= (int64_t)1 << 31 || nNodes >= ((int64_t)1 << 31) - 1)
		return fail("mesh connectivity: %lld triangles, %lld nodes", (long long)nTris, (long long)nNodes);
	const int64_t a = tmp_need(nTris, nNodes), b = kill_need(nTris, nNodes);
	*bytes_host = a > b ? a : b;
	return 0;
}

int mf_meshops_build(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int32_t* opposite, int32_t* nodeOff, int32_t* ringNodes,
                     int32_t* triOff, int32_t* ringTris, void* tmp, int64_t tmp_bytes, int32_t* out_host, void* stream) {
	MF_TRY(check_sizes("mesh connectivity", nTris, tcap, nNodes, nNodes));
	const hipStream_t st = (hipStream_t)stream;
	out_host[0] = out_host[1] = 0;
	out_host[2] = out_host[3] = -1;
	MF_HIP(hipMemsetAsync(nodeOff, 0, (nNodes + 1) * sizeof(int32_t), st));
	MF_HIP(hipMemsetAsync(triOff, 0, (nNodes + 1) * sizeof(int32_t), st));
	if (nTris == 0) return 0;
	const int64_t need = tmp_need(nTris, nNodes), n = 3 * nTris, m = 6 * nTris;
	HeadWs t;
	MF_TRY(head_ws_cut("mesh connectivity", tmp, tmp_bytes, need, &t));
	Cutter cut(t.ws, t.ws_bytes);
	uint32_t *k0, *k1;
	int32_t *v0, *v1;
	MF_TRY(cut.take((size_t)m, &k0, &k1));
	MF_TRY(cut.take((size_t)m, &v0, &v1));
	void* ws = cut.p;
	const size_t ws_bytes = cut.left;
	int32_t* head = (int32_t*)t.head;
	const Tris T = {nTris, tcap, nNodes, tri};
	const int bits = key_bits(nNodes);
	hipLaunchKernelGGL(k_head_init, dim3(1), dim3(64), 0, st, head);
	hipLaunchKernelGGL(k_validate, dim3(nblk(nTris)), dim3(BLOCK), 0, st, T, head);
	// the corner table: the corners sorted by (smaller, larger) node of their edge, ascending corner number within an edge
	hipLaunchKernelGGL(k_corner_keys, dim3(nblk(n)), dim3(BLOCK), 0, st, T, 0, k0, v0);
	MF_LAUNCH_CHECK();
	MF_TRY(sort_pairs(ws, ws_bytes, k0, k1, v0, v1, n, bits, st));
	hipLaunchKernelGGL(k_corner_lo, dim3(nblk(n)), dim3(BLOCK), 0, st, T, (const int32_t*)head, (const int32_t*)v1, k0);
	MF_LAUNCH_CHECK();
	MF_TRY(sort_pairs(ws, ws_bytes, k0, k1, v1, v0, n, bits, st));
	hipLaunchKernelGGL(k_groups, dim3(nblk(n)), dim3(BLOCK), 0, st, T, (const int32_t*)v0, opposite, head);
	// the triangles of the 1-rings: the corners sorted by their node
	hipLaunchKernelGGL(k_corner_keys, dim3(nblk(n)), dim3(BLOCK), 0, st, T, 1, k0, v1);
	MF_LAUNCH_CHECK();
	MF_TRY(sort_pairs(ws, ws_bytes, k0, k1, v1, v0, n, bits, st));
	hipLaunchKernelGGL(k_tri_csr, dim3(nblk(n)), dim3(BLOCK), 0, st, T, (const int32_t*)head, (const uint32_t*)k1, (const int32_t*)v0, triOff, ringTris);
	// the nodes of the 1-rings: the (node, neighbour) pairs sorted by node, then neighbour, the first of each kept
	hipLaunchKernelGGL(k_pair_keys, dim3(nblk(m)), dim3(BLOCK), 0, st, T, k0, v0);
	MF_LAUNCH_CHECK();
	MF_TRY(sort_pairs(ws, ws_bytes, k0, k1, v0, v1, m, bits, st));
	hipLaunchKernelGGL(k_pair_node, dim3(nblk(m)), dim3(BLOCK), 0, st, T, (const int32_t*)head, (const int32_t*)v1, k0);
	MF_LAUNCH_CHECK();
	MF_TRY(sort_pairs(ws, ws_bytes, k0, k1, v1, v0, m, bits, st));
	int32_t* rank = (int32_t*)k0;
	hipLaunchKernelGGL(k_pair_first, dim3(nblk(m)), dim3(BLOCK), 0, st, T, (const int32_t*)head, (const int32_t*)v0, rank);
	MF_LAUNCH_CHECK();
	MF_TRY(exclusive_sum(ws, ws_bytes, rank, rank, m, st));
	hipLaunchKernelGGL(k_ring_csr, dim3(nblk(m)), dim3(BLOCK), 0, st, T, (const int32_t*)head, (const uint32_t*)k1, (const int32_t*)v0, (const int32_t*)rank,
	                   nodeOff, ringNodes);
	MF_LAUNCH_CHECK();
	int32_t host[4] = {0, 0, 0, 0};
	MF_TRY(read_back(host, head, sizeof(host), st));
	out_host[0] = host[0];
	out_host[1] = host[1];
	out_host[2] = host[2] == INT_MAX ? -1 : host[2];
	out_host[3] = host[3] == INT_MAX ? -1 : host[3];
	return 0;
}

int mf_meshops_smooth_step(int64_t nNodes, int64_t ncap, float* pos, const int32_t* nflags, const int32_t* nodeOff, const int32_t* ringNodes,
                           const int32_t* triOff, float str, float minLength, float* temp, void* stream) {
	MF_TRY(check_sizes("smoothMesh", 0, 0, nNodes, ncap));
	if (nNodes == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	const Nodes N = {nNodes, ncap, pos, nflags};
	hipLaunchKernelGGL(k_smooth, dim3(nblk(nNodes)), dim3(BLOCK), 0, st, N, nodeOff, ringNodes, triOff, str, minLength, temp);
	hipLaunchKernelGGL(k_copy_back, dim3(nblk(nNodes)), dim3(BLOCK), 0, st, nNodes, ncap, pos, nflags, (const float*)temp);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_meshops_volume_terms(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, double* terms,
                            void* stream) {
	MF_TRY(check_sizes("computeCenterOfMass", nTris, tcap, nNodes, ncap));
	if (nTris == 0) return 0;
	const Tris T = {nTris, tcap, nNodes, tri};
	hipLaunchKernelGGL(k_volume_terms, dim3(nblk(nTris)), dim3(BLOCK), 0, (hipStream_t)stream, T, ncap, pos, terms);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_meshops_volume_sums(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, void* tmp,
                           int64_t tmp_bytes, double* sums_host, void* stream) {
	MF_TRY(check_sizes("computeCenterOfMass", nTris, tcap, nNodes, ncap));
	for (int q = 0; q < 4; q++) sums_host[q] = 0.;
	if (nTris == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	HeadWs t;
	MF_TRY(head_ws_cut("computeCenterOfMass", tmp, tmp_bytes, tmp_need(nTris, nNodes), &t));
	const int64_t nb = nblk(nTris);
	Cutter cut(t.ws, t.ws_bytes);
	double* part;
	MF_TRY(cut.take((size_t)(4 * nb), &part));
	const Tris T = {nTris, tcap, nNodes, tri};
	MF_TRY((reduce<SumF64, 4>(nTris, dim3((unsigned)nb), VolumeTerm{T, ncap, pos}, part, Store<double, 4>{(double*)t.head}, st)));
	return read_back(sums_host, t.head, 4 * sizeof(double), st);
}

int mf_meshops_rescale_scalars(const double* sums0_host, const double* sums1_host, float* out_host) {
	const double* sums[2] = {sums0_host, sums1_host};
	float vol[2];
	for (int w = 0; w < 2; w++) {
		double cm[3] = {sums[w][1], sums[w][2], sums[w][3]};
		if (sums[w][0] != 0.0)
			for (int c = 0; c < 3; c++) cm[c] /= sums[w][0];
		for (int c = 0; c < 3; c++) out_host[3 * w + c] = (float)cm[c];
		vol[w] = (float)sums[w][0];
	}
	out_host[6] = cbrtf(vol[0] / vol[1]);
	return 0;
}

int mf_meshops_rescale(int64_t nNodes, int64_t ncap, float* pos, const int32_t* nflags, float ox, float oy, float oz, float nx, float ny, float nz,
                       float beta, void* stream) {
	MF_TRY(check_sizes("smoothMesh", 0, 0, nNodes, ncap));
	if (nNodes == 0) return 0;
	hipLaunchKernelGGL(k_rescale, dim3(nblk(nNodes)), dim3(BLOCK), 0, (hipStream_t)stream, nNodes, ncap, pos, nflags, ox, oy, oz, nx, ny, nz, beta);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_meshops_kill_plan(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, const int32_t* opposite, int elements, void* tmp,
                         int64_t tmp_bytes, int32_t* out_host, void* stream) {
	MF_TRY(check_sizes("killSmallComponents", nTris, tcap, nNodes, nNodes));
	out_host[0] = out_host[1] = out_host[2] = out_host[3] = 0;
	out_host[4] = -1;
	if (nTris == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	KillWs w;
	MF_TRY(kill_cut(tmp, tmp_bytes, nTris, nNodes, &w));
	const Tris T = {nTris, tcap, nNodes, tri};
	const int64_t n = 3 * nTris;
	hipLaunchKernelGGL(k_fill_i32, dim3(nblk(nTris)), dim3(BLOCK), 0, st, nTris, w.label, 0, 1);
	MF_LAUNCH_CHECK();
	// a round that changes something lowers a label, so the rounds end; one int is read back per round
	int32_t changed = 1;
	while (changed) {
		MF_HIP(hipMemsetAsync(w.head, 0, sizeof(int32_t), st));
		hipLaunchKernelGGL(k_hook, dim3(nblk(nTris)), dim3(BLOCK), 0, st, nTris, opposite, w.label, w.head);
		hipLaunchKernelGGL(k_jump, dim3(nblk(nTris)), dim3(BLOCK), 0, st, nTris, w.label);
		MF_LAUNCH_CHECK();
		MF_TRY(read_back(&changed, w.head, sizeof(changed), st));
		out_host[0]++;
	}
	MF_HIP(hipMemsetAsync(w.head, 0, 8 * sizeof(int32_t), st));
	MF_HIP(hipMemsetAsync(w.size, 0, nTris * sizeof(int32_t), st));
	hipLaunchKernelGGL(k_fill_i32, dim3(1), dim3(BLOCK), 0, st, 1, w.head + 3, INT_MAX, 0);
	hipLaunchKernelGGL(k_fill_i32, dim3(nblk(nNodes)), dim3(BLOCK), 0, st, nNodes, w.first, INT_MAX, 0);
	hipLaunchKernelGGL(k_comp_sizes, dim3(nblk(nTris)), dim3(BLOCK), 0, st, nTris, (const int32_t*)w.label, w.size, w.head);
	hipLaunchKernelGGL(k_taint, dim3(nblk(nTris)), dim3(BLOCK), 0, st, nTris, (const int32_t*)w.label, (const int32_t*)w.size, elements, w.taint, w.head);
	hipLaunchKernelGGL(k_first_corner, dim3(nblk(n)), dim3(BLOCK), 0, st, T, (const int32_t*)w.taint, w.first);
	hipLaunchKernelGGL(k_shared_and_flags, dim3(nblk(n)), dim3(BLOCK), 0, st, T, (const int32_t*)w.taint, (const int32_t*)w.first, w.cflag, w.head);
	MF_LAUNCH_CHECK();
	MF_TRY(exclusive_sum(w.ws, w.ws_bytes, w.cflag, w.cflag, n, st));
	hipLaunchKernelGGL(k_deleted_list, dim3(nblk(n)), dim3(BLOCK), 0, st, T, (const int32_t*)w.taint, (const int32_t*)w.first, (const int32_t*)w.cflag, w.deleted,
	                   w.head);
	MF_LAUNCH_CHECK();
	MF_TRY(exclusive_sum(w.ws, w.ws_bytes, w.taint, w.below, nTris, st));
	int32_t host[5];
	MF_TRY(read_back(host, w.head, sizeof(host), st));
	out_host[1] = host[4];
	out_host[2] = host[1];
	out_host[3] = host[2];
	out_host[4] = host[3] == INT_MAX ? -1 : host[3];
	return 0;
}

int mf_meshops_kill_apply(int64_t nTris, int64_t tcap, int32_t* tri, int32_t* tflags, int64_t nNodes, int64_t ncap, float* pos, float* normal,
                          int32_t* nflags, int64_t killedTris, int64_t deletedNodes, void* tmp, int64_t tmp_bytes, void* stream) {
	MF_TRY(check_sizes("killSmallComponents", nTris, tcap, nNodes, ncap));
	const int64_t K = killedTris, D = deletedNodes;
	if (K < 0 || K > nTris || D < 0 || D > nNodes) return fail("killSmallComponents: %lld of %lld triangles, %lld of %lld nodes", (long long)K, (long long)nTris, (long long)D, (long long)nNodes);
	if (K == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	KillWs w;
	MF_TRY(kill_cut(tmp, tmp_bytes, nTris, nNodes, &w));
	const int64_t newT = nTris - K, newsize = nNodes - D;
	if (newT > 0) {
		hipLaunchKernelGGL(k_fill_holes, dim3(nblk(newT)), dim3(BLOCK), 0, st, nTris, tcap, (int32_t)K, (const int32_t*)w.taint, (const int32_t*)w.below, tri, tflags);
		MF_LAUNCH_CHECK();
	}
	if (D == 0) return 0;
	hipLaunchKernelGGL(k_node_flags, dim3(nblk(D)), dim3(BLOCK), 0, st, D, newsize, (const int32_t*)w.deleted, (const int32_t*)w.first, w.spotFlag, w.keptFlag);
	MF_LAUNCH_CHECK();
	MF_TRY(exclusive_sum(w.ws, w.ws_bytes, w.spotFlag, w.spotRank, D, st));
	MF_TRY(exclusive_sum(w.ws, w.ws_bytes, w.keptFlag, w.keptRank, D, st));
	hipLaunchKernelGGL(k_spots, dim3(nblk(D)), dim3(BLOCK), 0, st, D, (const int32_t*)w.deleted, (const int32_t*)w.spotFlag, (const int32_t*)w.spotRank, w.spot);
	hipLaunchKernelGGL(k_move_nodes, dim3(nblk(D)), dim3(BLOCK), 0, st, D, newsize, ncap, (const int32_t*)w.keptFlag, (const int32_t*)w.keptRank,
	                   (const int32_t*)w.spot, w.newIndex, pos, normal, nflags);
	if (newT > 0) hipLaunchKernelGGL(k_remap_tris, dim3(nblk(3 * newT)), dim3(BLOCK), 0, st, newT, tcap, newsize, D, (const int32_t*)w.newIndex, tri);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
