// mesh.hip -- surface meshes (include/open/manta_hip_mesh.h): marching cubes as classify -> count -> scan -> emit with one thread per
// cell and lanes along x, the node advection of Mesh::advectInGrid with one thread per node, and the element-wise node transforms.
// The per-cell bodies are in mesh_cells.h.  Reference: levelset.cpp:330-415, mesh.cpp:301-373, util/integrator.h:26-78.
#include "mesh_cells.h"
#include "../../include/open/manta_hip_mesh.h"
#include "scan.h"

using namespace mf;
using namespace mf::mesh;

namespace {

__global__ void __launch_bounds__(BLOCK) k_classify(Dim d, const float* __restrict__ phi, uint8_t* __restrict__ cube) {
	CELL_IJK(d)
	cube[idx] = (uint8_t)classify_cell(d, phi, i, j, k);
}

__global__ void __launch_bounds__(BLOCK)
k_count(Dim d, const uint8_t* __restrict__ cube, uint16_t* __restrict__ mask, int32_t* __restrict__ nodeCnt, int32_t* __restrict__ triCnt) {
	CELL_IJK(d)
	const unsigned c = cube[idx];
	const unsigned m = c ? owned_mask(d, cube, i, j, k, c) : 0u;
	mask[idx] = (uint16_t)m;
	nodeCnt[idx] = __builtin_popcount(m);
	triCnt[idx] = c ? tri_count(c) : 0;
}

// the totals from the last cell: its exclusive offsets plus its own counts (the last cell of a grid is never active, but nothing here
// depends on that)
__global__ void k_totals(int64_t n, const uint8_t* __restrict__ cube, const uint16_t* __restrict__ mask, const int32_t* __restrict__ nodeOff,
                         const int32_t* __restrict__ triOff, int64_t* __restrict__ res) {
	if (blockIdx.x || threadIdx.x) return;
	const unsigned c = cube[n - 1];
	res[0] = (int64_t)nodeOff[n - 1] + __builtin_popcount((unsigned)mask[n - 1]);
	res[1] = (int64_t)triOff[n - 1] + (c ? tri_count(c) : 0);
}

__global__ void __launch_bounds__(BLOCK)
k_emit(Dim d, const float* __restrict__ phi, const uint8_t* __restrict__ cube, const uint16_t* __restrict__ mask,
       const int32_t* __restrict__ nodeOff, const int32_t* __restrict__ triOff, MeshOut M) {
	CELL_IJK(d)
	emit_cell(d, phi, cube, mask, nodeOff, triOff, i, j, k, M);
}

// KnAdvectMeshInGrid, mesh.cpp:301-309
__device__ __forceinline__ void node_velocity(const Dim& d, const float* __restrict__ vel, bool fixed, float dt, const float x[3], float u[3]) {
	if (fixed || !in_bounds_pos(d, x[0], x[1], x[2], 1)) {
		u[0] = u[1] = u[2] = 0.f;
		return;
	}
	float vx, vy, vz;
	interpol_mac(d, vel, x[0], x[1], x[2], vx, vy, vz);
	u[0] = vx * dt;
	u[1] = vy * dt;
	u[2] = vz * dt;
}
// the host-side loops of integratePointSet (integrator.h:26-78, with the fork's `uTotal += u` at line 55) fused: nodes are independent
__global__ void __launch_bounds__(BLOCK)
k_advect(Dim d, const float* __restrict__ vel, int64_t n, int64_t ncap, float* __restrict__ pos, const int32_t* __restrict__ nflags, float dt, int mode) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= n) return;
	const bool fixed = (nflags[p] & 1) != 0;     // Mesh::NfFixed
	const float x0[3] = {pos[p], pos[ncap + p], pos[2 * ncap + p]};
	float x[3] = {x0[0], x0[1], x0[2]}, u[3];
	node_velocity(d, vel, fixed, dt, x, u);
	if (mode == MF_INT_EULER) {
		for (int c = 0; c < 3; c++) x[c] = x[c] + u[c];
	} else if (mode == MF_INT_RK2) {
		for (int c = 0; c < 3; c++) x[c] = x0[c] + 0.5f * u[c];
		node_velocity(d, vel, fixed, dt, x, u);
		for (int c = 0; c < 3; c++) x[c] = x0[c] + u[c];
	} else {
		float ut[3];
		for (int c = 0; c < 3; c++) {
			ut[c] = u[c];
			x[c] = x0[c] + 0.5f * u[c];
			ut[c] = ut[c] + u[c];
		}
		node_velocity(d, vel, fixed, dt, x, u);
		for (int c = 0; c < 3; c++) {
			x[c] = x0[c] + 0.5f * u[c];
			ut[c] = ut[c] + 2.f * u[c];
		}
		node_velocity(d, vel, fixed, dt, x, u);
		for (int c = 0; c < 3; c++) {
			x[c] = x0[c] + u[c];
			ut[c] = ut[c] + 2.f * u[c];
		}
		node_velocity(d, vel, fixed, dt, x, u);
		const float sixth = (float)(1. / 6.);
		for (int c = 0; c < 3; c++) x[c] = x0[c] + sixth * (ut[c] + u[c]);
	}
	pos[p] = x[0];
	pos[ncap + p] = x[1];
	pos[2 * ncap + p] = x[2];
}

template <bool MUL>
__global__ void __launch_bounds__(BLOCK) k_scale_offset(int64_t n, int64_t ncap, float* __restrict__ pos, float x, float y, float z) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= n) return;
	const float v[3] = {x, y, z};
	for (int c = 0; c < 3; c++) pos[c * ncap + p] = MUL ? pos[c * ncap + p] * v[c] : pos[c * ncap + p] + v[c];
}

__global__ void __launch_bounds__(BLOCK) k_rotate_pair(int64_t n, float* __restrict__ a, float* __restrict__ b, float sin_t, float cos_t) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= n) return;
	rotate_pair(a + p, b + p, sin_t, cos_t);
}

int check_mesh_grid(const char* who, int sx, int sy, int sz) {
	MF_TRY(check_dim(sx, sy, sz));
	if (sz == 1) return fail("Only 3D grids supported so far");
	if (sx < 3 || sy < 3 || sz < 3) return fail("%s: grid %dx%dx%d is thinner than 3 cells (getGradient would read outside it)", who, sx, sy, sz);
	if ((int64_t)sx * sy * sz * 5 >= (int64_t)1 << 31) return fail("%s: grid too large for 32-bit node and triangle numbers", who);
	if (g_slab_gsz > 0) return fail("%s: not available inside a z-slab window", who);
	return 0;
}
int check_nodes(const char* who, int64_t n, int64_t ncap) {
	if (n < 0 || ncap < n) return fail("%s: %lld nodes in arrays of stride %lld", who, (long long)n, (long long)ncap);
	return 0;
}

}  // namespace

extern "C" {

int mf_mesh_abi_version(void) { return MF_MESH_ABI_VERSION; }

int mf_mesh_scan_bytes(int sx, int sy, int sz, int64_t* bytes_host) {
	MF_TRY(check_mesh_grid("createMesh", sx, sy, sz));
	size_t b = 0;
	MF_TRY(exclusive_sum32_bytes((int64_t)sx * sy * sz, &b));
	*bytes_host = head_ws_bytes(b);
	return 0;
}

int mf_mesh_create_plan(int sx, int sy, int sz, const float* phi, void* cube, void* mask, int32_t* nodeOff, int32_t* triOff, void* tmp,
                        int64_t tmp_bytes, int64_t* totals_host, void* stream) {
	int64_t need = 0;
	MF_TRY(mf_mesh_scan_bytes(sx, sy, sz, &need));
	const Dim d = mkdim(sx, sy, sz);
	const hipStream_t st = (hipStream_t)stream;
	HeadWs t;
	MF_TRY(head_ws_cut("createMesh", tmp, tmp_bytes, need, &t));
	hipLaunchKernelGGL(k_classify, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, phi, (uint8_t*)cube);
	hipLaunchKernelGGL(k_count, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, (const uint8_t*)cube, (uint16_t*)mask, nodeOff, triOff);
	MF_LAUNCH_CHECK();
	MF_TRY(exclusive_sum(t.ws, t.ws_bytes, nodeOff, nodeOff, d.n, st));
	MF_TRY(exclusive_sum(t.ws, t.ws_bytes, triOff, triOff, d.n, st));
	hipLaunchKernelGGL(k_totals, dim3(1), dim3(64), 0, st, d.n, (const uint8_t*)cube, (const uint16_t*)mask, nodeOff, triOff, t.head);
	MF_LAUNCH_CHECK();
	return read_back(totals_host, t.head, 2 * sizeof(int64_t), st);
}

int mf_mesh_create_emit(int sx, int sy, int sz, const float* phi, const void* cube, const void* mask, const int32_t* nodeOff,
                        const int32_t* triOff, int64_t nNodes, int64_t nTris, int64_t ncap, float* pos, float* normal, int32_t* nflags,
                        int64_t tcap, int32_t* tri, int32_t* tflags, void* stream) {
	MF_TRY(check_mesh_grid("createMesh", sx, sy, sz));
	if (nNodes < 0 || nTris < 0 || ncap < nNodes || tcap < nTris)
		return fail("createMesh: %lld nodes / %lld triangles in arrays of stride %lld / %lld", (long long)nNodes, (long long)nTris, (long long)ncap, (long long)tcap);
	if (nNodes == 0 && nTris == 0) return 0;
	const Dim d = mkdim(sx, sy, sz);
	const MeshOut M = {nNodes, nTris, ncap, tcap, pos, normal, nflags, tri, tflags};
	hipLaunchKernelGGL(k_emit, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, phi, (const uint8_t*)cube, (const uint16_t*)mask, nodeOff, triOff, M);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mesh_advect(int sx, int sy, int sz, const float* vel, int64_t n, int64_t ncap, float* pos, const int32_t* nflags, float dt,
                   int integrationMode, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("Mesh::advectInGrid: not available inside a z-slab window");
	if (integrationMode < 0 || integrationMode > 2) return fail("unknown integration type");
	MF_TRY(check_nodes("Mesh::advectInGrid", n, ncap));
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_advect, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, mkdim(sx, sy, sz), vel, n, ncap, pos, nflags, dt, integrationMode);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mesh_scale(int64_t n, int64_t ncap, float* pos, float x, float y, float z, void* stream) {
	MF_TRY(check_nodes("Mesh::scale", n, ncap));
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_scale_offset<true>, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, ncap, pos, x, y, z);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mesh_offset(int64_t n, int64_t ncap, float* pos, float x, float y, float z, void* stream) {
	MF_TRY(check_nodes("Mesh::offset", n, ncap));
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_scale_offset<false>, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, ncap, pos, x, y, z);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mesh_rotate_pair(int64_t n, int64_t ncap, float* pos, int first, int second, float sin_t, float cos_t, void* stream) {
	MF_TRY(check_nodes("Mesh::rotate", n, ncap));
	if (first < 0 || first > 2 || second < 0 || second > 2 || first == second) return fail("Mesh::rotate: invalid axis pair %d, %d", first, second);
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_rotate_pair, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, pos + first * ncap, pos + second * ncap, sin_t, cos_t);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mesh_sincos(float theta, float* sin_host, float* cos_host) {
	*sin_host = sinf(theta);
	*cos_host = cosf(theta);
	return 0;
}

}  // extern "C"
