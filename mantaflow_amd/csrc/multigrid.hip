// multigrid.hip -- the multigrid preconditioner of the pressure PCG on gfx950, 3-D (include/manta_hip_multigrid.h): the
// description of the 3-D hierarchy for the driver they share (mg_driver.h: handle, kernels, tail, set-up, V-cycle, entry
// bodies) and the C entries.  The per-vertex bodies are mg3d_cells.h.  The 2-D hierarchy is mg2d.hip, over the same driver.
// Reference: source/multigrid.{h,cpp} (GridMg, cited per function), source/conjugategrad.cpp:100-106, 162-167 (PC_MGP).
#include "mg3d_cells.h"
#include "mg_driver.h"
#include "../../include/manta_hip_multigrid.h"

using namespace mf;

namespace {

struct Mg3d {
	using Lv = mg3d::Lv;
	using View = mg3d::View;
	using Path = mg3d::Path;
	struct Coord {
		int X, Y, Z;
	};
	static constexpr unsigned MAGIC = 0x4d474d47u;
	static constexpr const char* NAME = "mf_mg";

	static int check_create(int, int, int sz) {
		if (sz <= 1) return fail("mf_mg_create: 2-D grids are not supported by the multigrid preconditioner on this backend (3-D only)");
		return 0;
	}
	static int pyramid(int sx, int sy, int sz, Lv* lv) {
		int sizes[MAXL][3];
		const int nl = mg3d::pyramid(sx, sy, sz, sizes);
		for (int l = 0; l < nl; l++) {
			lv[l].sx = sizes[l][0];
			lv[l].sy = sizes[l][1];
			lv[l].sz = sizes[l][2];
			lv[l].n = sizes[l][0] * sizes[l][1] * sizes[l][2];
		}
		return nl;
	}
	static SizeStr size_str(const MgDim& d) {
		SizeStr o;
		snprintf(o.s, sizeof o.s, "%d x %d x %d", d.sx, d.sy, d.sz);
		return o;
	}
	static int planes(bool l0) { return l0 ? 4 : 14; }
	static MG_HD int smooth_colours(bool l0) { return mg3d::smooth_colours(l0); }
	static std::vector<Path> make_paths() { return mg3d::make_paths(); }
	static MG_HD Coord coord(const Lv& L, int v) { return Coord{v % L.sx, (v / L.sx) % L.sy, v / (L.sx * L.sy)}; }
	static MG_HD double cg_apply(const Lv& L, bool l0, int v, const Coord& c, const double* vec) { return mg3d::cg_apply(L, l0, v, c.X, c.Y, c.Z, vec); }
	static MG_HD void copy_activate(const Lv& L, int v, const float* A0, const float* Ai, const float* Aj, const float* Ak, int* info) {
		mg3d::copy_activate(L, v, A0, Ai, Aj, Ak, info);
	}
};

}  // namespace

// what mgslab.hip borrows of a live handle (mg3d_cells.h)
namespace mf {
namespace mg3d {
static int live3d(void* handle, const char* who, Mg<Mg3d>** out) {
	Mg<Mg3d>* m = as_mg<Mg3d>(handle);
	if (!m) return fail("%s: bad handle (not a live 3-D hierarchy of mf_mg_create)", who);
	if (!m->aset) return fail("%s: GridMg::setRhs Error: A has not been set.", who);
	*out = m;
	return 0;
}
int borrow(void* handle, const char* who, Borrowed* out) {
	Mg<Mg3d>* m;
	MF_TRY(live3d(handle, who, &m));
	out->v = m->v;
	out->tail_first = m->tail_first;
	return 0;
}
int coarse_cycle(void* handle, const char* who, hipStream_t st) {
	Mg<Mg3d>* m;
	MF_TRY(live3d(handle, who, &m));
	if (m->tail_first < 1)
		return fail("%s: level 0 of this hierarchy runs inside the single-workgroup tail (mf_mg_info slot [5] == 0): it is not cut, use mf_mg_vcycle", who);
	// knSet(x_1, 0), multigrid.cpp:472: whole, whatever coarse planes the caller restricted into
	MF_HIP(hipMemsetAsync(m->v.l[1].x, 0, sizeof(float) * m->v.l[1].n, st));
	levels_down_up(m, 1, st);
	MF_LAUNCH_CHECK();
	return 0;
}
int set_solve_accuracy(void* handle, const char* who, float accuracy) {
	Mg<Mg3d>* m;
	MF_TRY(live3d(handle, who, &m));
	m->coarsestAcc = (float)(accuracy * 1E-4);
	return 0;
}
}  // namespace mg3d
}  // namespace mf

extern "C" {

int mf_multigrid_abi_version(void) { return MF_MULTIGRID_ABI_VERSION; }

int mf_mg_create(int sx, int sy, int sz, void** handle_out) { return mg_create<Mg3d>(sx, sy, sz, handle_out); }
int mf_mg_destroy(void* handle) { return mg_destroy<Mg3d>(handle); }
int mf_mg_set_a(void* handle, const float* A0, const float* Ai, const float* Aj, const float* Ak, void* stream) {
	return mg_set_a<Mg3d>(handle, A0, Ai, Aj, Ak, stream);
}
int mf_mg_is_a_set(void* handle) { return mg_is_a_set<Mg3d>(handle); }
int mf_mg_vcycle(void* handle, float* dst, const float* rhs, void* stream) { return mg_vcycle<Mg3d>(handle, dst, rhs, stream); }
int mf_mg_cg_solve(void* handle, int sx, int sy, int sz, const int32_t* flags, float* dst, const float* rhs, float* residual,
                   float* search, float* tmp, const float* A0, const float* Ai, const float* Aj, const float* Ak, float accuracy,
                   int maxIter, int useL2Norm, float* out_host, void* stream) {
	return mg_cg_solve<Mg3d>(handle, sx, sy, sz, flags, dst, rhs, residual, search, tmp, A0, Ai, Aj, Ak, accuracy, maxIter, useL2Norm, out_host, stream);
}
int mf_mg_info(void* handle, int64_t* out_host, int n_out) { return mg_info<Mg3d>(handle, out_host, n_out); }
int mf_mg_read_level(void* handle, int level, int what, void* dst_host, int64_t bytes) { return mg_read_level<Mg3d>(handle, level, what, dst_host, bytes); }

}  // extern "C"
