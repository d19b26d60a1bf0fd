// mgslab.hip -- the V-cycle of the 3-D multigrid preconditioner with level 0 cut into ranges of z-planes, for the z-slab pressure
// solve (include/open/manta_hip_mgslab.h).  It works on the handles of mf_mg_create: multigrid.hip owns the registry of live
// handles and the kernels of the driver, and lends the levels of a handle, the replicated levels 1 .. L-1 and the accuracy
// setter through the three functions at the end of mg3d_cells.h.  The kernels here are the ranged forms of the level-0 passes:
// the per-vertex bodies of mg3d_cells.h on the work items [begin, end), one item per thread -- the same definitions the
// whole-grid kernels and the tail of mg_driver.h run, so a plane comes out with the same bits whoever computes it.
// Reference: source/multigrid.{h,cpp} (GridMg, cited per function in mg3d_cells.h).
#include "mg3d_cells.h"
#include "../../include/open/manta_hip_mgslab.h"

using namespace mf;
using mg3d::Borrowed;
using mg3d::Lv;

namespace {

// knSetRhs + knSet(x_0, 0) on the vertices [begin, end); rhs holds those vertices only
__global__ void __launch_bounds__(BLOCK) k_mgslab_set_rhs(Lv L, const float* __restrict__ rhs, int begin, int end) {
	const int v = begin + blockIdx.x * BLOCK + threadIdx.x;
	if (v < end) set_rhs(L, v, rhs - begin);
}
__global__ void __launch_bounds__(BLOCK) k_mgslab_smooth(Lv L, int colour, int begin, int end) {
	mg3d::pass_smooth(L, true, colour, begin, end, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK);
}
__global__ void __launch_bounds__(BLOCK) k_mgslab_residual(Lv L, int begin, int end) {
	mg3d::pass_residual(L, true, begin, end, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK);
}
__global__ void __launch_bounds__(BLOCK) k_mgslab_restrict(Lv F, Lv C, int begin, int end) {
	mg3d::pass_restrict(F, C, begin, end, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK);
}
__global__ void __launch_bounds__(BLOCK) k_mgslab_interp_add(Lv F, Lv C, int begin, int end) {
	mg3d::pass_interp_add(F, C, begin, end, blockIdx.x * BLOCK + threadIdx.x, gridDim.x * BLOCK);
}

// the handle's levels, and the plane range [z0, z1) of level `level` checked against it.  A level has fewer than 2^31 vertices
// (check_dim at mf_mg_create), so item ranges are ints.
int borrow_range(void* handle, const char* who, int level, int z0, int z1, Borrowed* B) {
	MF_TRY(mg3d::borrow(handle, who, B));
	if (level < 0 || level >= B->v.nl) return fail("%s: level %d of %d", who, level, B->v.nl);
	const int sz = B->v.l[level].sz;
	if (z0 < 0 || z1 > sz || z0 > z1) return fail("%s: plane range [%d, %d) outside the %d planes of level %d", who, z0, z1, sz, level);
	return 0;
}
// the cut form restricts into, and interpolates from, level 1
int need_level1(const Borrowed& B, const char* who) {
	if (B.v.nl < 2) return fail("%s: the hierarchy has one level: there is no level 1 to cut against, use mf_mg_vcycle", who);
	return 0;
}
int plane_of(const Lv& L) { return L.sx * L.sy; }

int copy_planes(void* handle, const char* who, int level, int what, int z0, int z1, float* out, const float* in, void* stream) {
	Borrowed B;
	MF_TRY(borrow_range(handle, who, level, z0, z1, &B));
	const Lv& L = B.v.l[level];
	float* vec = what == 2 ? L.x : what == 3 ? L.b : what == 4 ? L.r : nullptr;
	if (!vec) return fail("%s: what = %d (2 x, 3 b, 4 r)", who, what);
	if (z0 == z1) return 0;
	if (!out && !in) return fail("%s: null tensor", who);
	const size_t XY = (size_t)plane_of(L), bytes = sizeof(float) * XY * (size_t)(z1 - z0);
	if (out) MF_HIP(hipMemcpyAsync(out, vec + XY * z0, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
	else MF_HIP(hipMemcpyAsync(vec + XY * z0, in, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
	return 0;
}

}  // namespace

extern "C" {

int mf_mgslab_abi_version(void) { return MF_MGSLAB_ABI_VERSION; }

int mf_mgslab_set_accuracy(void* handle, float accuracy) { return mg3d::set_solve_accuracy(handle, "mf_mgslab_set_accuracy", accuracy); }

int mf_mgslab_set_rhs(void* handle, int z0, int z1, const float* rhs, void* stream) {
	Borrowed B;
	MF_TRY(borrow_range(handle, "mf_mgslab_set_rhs", 0, z0, z1, &B));
	if (z0 == z1) return 0;
	if (!rhs) return fail("mf_mgslab_set_rhs: null rhs");
	const Lv& L = B.v.l[0];
	const int XY = plane_of(L);
	hipStream_t st = (hipStream_t)stream;
	if (z0 > 0) MF_HIP(hipMemsetAsync(L.x + (size_t)XY * (z0 - 1), 0, sizeof(float) * XY, st));
	if (z1 < L.sz) MF_HIP(hipMemsetAsync(L.x + (size_t)XY * z1, 0, sizeof(float) * XY, st));
	hipLaunchKernelGGL(k_mgslab_set_rhs, dim3(nblk((int64_t)XY * (z1 - z0))), dim3(BLOCK), 0, st, L, rhs, XY * z0, XY * z1);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mgslab_smooth(void* handle, int colour, int z0, int z1, void* stream) {
	Borrowed B;
	MF_TRY(borrow_range(handle, "mf_mgslab_smooth", 0, z0, z1, &B));
	if (colour != 0 && colour != 1) return fail("mf_mgslab_smooth: colour %d (level 0 has the colours 0 and 1)", colour);
	if (z0 == z1) return 0;
	const Lv& L = B.v.l[0];
	const int per = ((L.sx + 1) >> 1) * L.sy;      // items of a plane (mg3d::smooth_items)
	hipLaunchKernelGGL(k_mgslab_smooth, dim3(nblk((int64_t)per * (z1 - z0))), dim3(BLOCK), 0, (hipStream_t)stream, L, colour, per * z0, per * z1);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mgslab_residual(void* handle, int z0, int z1, void* stream) {
	Borrowed B;
	MF_TRY(borrow_range(handle, "mf_mgslab_residual", 0, z0, z1, &B));
	if (z0 == z1) return 0;
	const Lv& L = B.v.l[0];
	const int XY = plane_of(L);
	hipLaunchKernelGGL(k_mgslab_residual, dim3(nblk((int64_t)XY * (z1 - z0))), dim3(BLOCK), 0, (hipStream_t)stream, L, XY * z0, XY * z1);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mgslab_restrict(void* handle, int k0, int k1, void* stream) {
	Borrowed B;
	MF_TRY(mg3d::borrow(handle, "mf_mgslab_restrict", &B));
	MF_TRY(need_level1(B, "mf_mgslab_restrict"));
	MF_TRY(borrow_range(handle, "mf_mgslab_restrict", 1, k0, k1, &B));
	if (k0 == k1) return 0;
	const Lv& C = B.v.l[1];
	const int XY = plane_of(C);
	hipLaunchKernelGGL(k_mgslab_restrict, dim3(nblk((int64_t)XY * (k1 - k0))), dim3(BLOCK), 0, (hipStream_t)stream, B.v.l[0], C, XY * k0, XY * k1);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mgslab_coarse(void* handle, void* stream) { return mg3d::coarse_cycle(handle, "mf_mgslab_coarse", (hipStream_t)stream); }

int mf_mgslab_interp_add(void* handle, int z0, int z1, void* stream) {
	Borrowed B;
	MF_TRY(borrow_range(handle, "mf_mgslab_interp_add", 0, z0, z1, &B));
	MF_TRY(need_level1(B, "mf_mgslab_interp_add"));
	if (z0 == z1) return 0;
	const Lv& L = B.v.l[0];
	const int XY = plane_of(L);
	hipLaunchKernelGGL(k_mgslab_interp_add, dim3(nblk((int64_t)XY * (z1 - z0))), dim3(BLOCK), 0, (hipStream_t)stream, L, B.v.l[1], XY * z0, XY * z1);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_mgslab_get_planes(void* handle, int level, int what, int z0, int z1, float* dst, void* stream) {
	return copy_planes(handle, "mf_mgslab_get_planes", level, what, z0, z1, dst, nullptr, stream);
}
int mf_mgslab_put_planes(void* handle, int level, int what, int z0, int z1, const float* src, void* stream) {
	return copy_planes(handle, "mf_mgslab_put_planes", level, what, z0, z1, nullptr, src, stream);
}

}  // extern "C"
