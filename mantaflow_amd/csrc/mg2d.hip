// mg2d.hip -- the multigrid preconditioner of the pressure PCG on 2-D grids, gfx950 (include/open/manta_hip_mg2d.h): the
// description of the 2-D hierarchy (GridMg with mIs3D == false) for the driver it shares with the 3-D one of multigrid.hip
// (mg_driver.h: handle, kernels, tail, set-up, V-cycle, entry bodies) and the C entries.  The per-vertex bodies are
// mg2d_cells.h.  A 2-D system is the driver's with sz = 1 and no Ak; its levels keep their own layout (3 / 5 planes).
// Reference: source/multigrid.{h,cpp} (cited per function in mg2d_cells.h), source/conjugategrad.cpp:100-106, 162-167 (PC_MGP).
#include "mg2d_cells.h"
#include "mg_driver.h"
#include "../../include/open/manta_hip_mg2d.h"

using namespace mf;

namespace {

struct Mg2d {
	using Lv = mg2d::Lv;
	using View = mg2d::View;
	using Path = mg2d::Path;
	struct Coord {
		int X, Y;
	};
	static constexpr unsigned MAGIC = 0x4d473244u;
	static constexpr const char* NAME = "mf_mg2d";

	static int check_create(int, int, int) { return 0; }
	static int pyramid(int sx, int sy, int, Lv* lv) {
		int sizes[MAXL][2];
		const int nl = mg2d::pyramid(sx, sy, sizes);
		for (int l = 0; l < nl; l++) {
			lv[l].sx = sizes[l][0];
			lv[l].sy = sizes[l][1];
			lv[l].n = sizes[l][0] * sizes[l][1];
		}
		return nl;
	}
	static SizeStr size_str(const MgDim& d) {
		SizeStr o;
		snprintf(o.s, sizeof o.s, "%d x %d", d.sx, d.sy);
		return o;
	}
	static int planes(bool l0) { return l0 ? 3 : 5; }
	static MG_HD int smooth_colours(bool l0) { return mg2d::smooth_colours(l0); }
	static std::vector<Path> make_paths() { return mg2d::make_paths(); }
	static MG_HD Coord coord(const Lv& L, int v) { return Coord{v % L.sx, v / L.sx}; }
	static MG_HD double cg_apply(const Lv& L, bool l0, int v, const Coord& c, const double* vec) { return mg2d::cg_apply(L, l0, v, c.X, c.Y, vec); }
	// PcExternal hands four planes over; a 2-D system has no Ak and the hierarchy does not look at it
	static MG_HD void copy_activate(const Lv& L, int v, const float* A0, const float* Ai, const float* Aj, const float*, int* info) {
		mg2d::copy_activate(L, v, A0, Ai, Aj, info);
	}
};

}  // namespace

extern "C" {

int mf_mg2d_abi_version(void) { return MF_MG2D_ABI_VERSION; }

int mf_mg2d_create(int sx, int sy, void** handle_out) { return mg_create<Mg2d>(sx, sy, 1, handle_out); }
int mf_mg2d_destroy(void* handle) { return mg_destroy<Mg2d>(handle); }
int mf_mg2d_set_a(void* handle, const float* A0, const float* Ai, const float* Aj, void* stream) {
	return mg_set_a<Mg2d>(handle, A0, Ai, Aj, nullptr, stream);
}
int mf_mg2d_is_a_set(void* handle) { return mg_is_a_set<Mg2d>(handle); }
int mf_mg2d_vcycle(void* handle, float* dst, const float* rhs, void* stream) { return mg_vcycle<Mg2d>(handle, dst, rhs, stream); }
int mf_mg2d_cg_solve(void* handle, int sx, int sy, const int32_t* flags, float* dst, const float* rhs, float* residual,
                     float* search, float* tmp, const float* A0, const float* Ai, const float* Aj, float accuracy,
                     int maxIter, int useL2Norm, float* out_host, void* stream) {
	return mg_cg_solve<Mg2d>(handle, sx, sy, 1, flags, dst, rhs, residual, search, tmp, A0, Ai, Aj, nullptr, accuracy, maxIter, useL2Norm, out_host, stream);
}
int mf_mg2d_info(void* handle, int64_t* out_host, int n_out) { return mg_info<Mg2d>(handle, out_host, n_out); }
int mf_mg2d_read_level(void* handle, int level, int what, void* dst_host, int64_t bytes) { return mg_read_level<Mg2d>(handle, level, what, dst_host, bytes); }

}  // extern "C"
