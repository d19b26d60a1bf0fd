/*
 * tools/vortex_record.cpp -- the C++ half of the recorder of tests/golden/vortex.npz (tools/record_vortex.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / VortexParticleSystem /
 * Mesh / Grid objects around caller-owned arrays and calls the reference's own advectSelf, applyToMesh, VPseedK41, markAsFixed and
 * densityFromLevelset.  The velocity kernels KnVpAdvectSelf / KnVpAdvectMesh are local to the reference's vortexpart.cpp, so the
 * recorder's commands put the `prep`-expanded file on the include path and this file includes it; plugin/vortexplugins.cpp is not part
 * of oracle/ref.mk's library and is expanded into a scratch directory and compiled next to this file.  Linked against
 * oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled with is committed.
 */
#include "vortexpart.cpp"      // the expanded reference source, from the build tree of oracle/ref.mk (-I)
#include "manta.h"
#include "grid.h"
#include "levelset.h"
#include "mesh.h"
#include "particle.h"
#include "shapes.h"
#include <cstring>
#include <memory>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void VPseedK41(VortexParticleSystem& system, const Shape* shape, Real strength, Real sigma0, Real sigma1, Real probability, Real N);
void markAsFixed(Mesh& mesh, const Shape* shape, bool exclusive);
void densityFromLevelset(const LevelsetGrid& phi, Grid<Real>& density, Real value, Real sigma);
}  // namespace Manta

using namespace Manta;

static std::string g_err;
#define REC_TRY try {
#define REC_CATCH                \
	}                            \
	catch (std::exception & e) { \
		g_err = e.what();        \
		return 1;                \
	}                            \
	return 0;

namespace {

// rows are AoS: pos[n][3], vort[n][3]
void fill(VortexParticleSystem& sys, int64_t n, const float* pos, const float* vort, const float* sigma, const int32_t* flag) {
	for (int64_t i = 0; i < n; i++) {
		sys.add(VortexParticleData(Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), Vec3(vort[3 * i], vort[3 * i + 1], vort[3 * i + 2]), sigma[i]));
		sys[i].flag = flag[i];
	}
}
void fill(std::vector<VortexParticleData>& v, int64_t n, const float* pos, const float* vort, const float* sigma, const int32_t* flag) {
	for (int64_t i = 0; i < n; i++) {
		v.push_back(VortexParticleData(Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), Vec3(vort[3 * i], vort[3 * i + 1], vort[3 * i + 2]), sigma[i]));
		v[i].flag = flag[i];
	}
}
void fill(Mesh& mesh, int64_t n, const float* pos, const int32_t* flags) {
	for (int64_t i = 0; i < n; i++) {
		mesh.addNode(Node(Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2])));
		mesh.nodes(i).flags = flags[i];
	}
}
std::unique_ptr<Shape> make_shape(FluidSolver* s, int kind, const float* a, const float* b) {
	if (kind == 0) return std::unique_ptr<Shape>(new Box(s, Vec3::Invalid, Vec3(a[0], a[1], a[2]), Vec3(b[0], b[1], b[2]), Vec3::Invalid));
	return std::unique_ptr<Shape>(new Sphere(s, Vec3(a[0], a[1], a[2]), b[0], Vec3(1, 1, 1)));
}
int64_t read_system(VortexParticleSystem& sys, int64_t cap, float* pos, float* vort, float* sigma, int32_t* flag) {
	const int64_t n = sys.size();
	if (n > cap) throw std::runtime_error("vortex_record: capacity too small");
	for (int64_t i = 0; i < n; i++) {
		for (int c = 0; c < 3; c++) {
			pos[3 * i + c] = sys[i].pos[c];
			vort[3 * i + c] = sys[i].vorticity[c];
		}
		sigma[i] = sys[i].sigma;
		flag[i] = sys[i].flag;
	}
	return n;
}

// the seeding stage: one solver per case, the stream is the reference's static
std::unique_ptr<FluidSolver> g_solver;
std::unique_ptr<VortexParticleSystem> g_sys;

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* one evaluation of the velocity kernels: u[nT][3].  self != 0: the particles are the targets (tpos, tflag unused) */
int rec_velocity(int self, int64_t nT, const float* tpos, const int32_t* tflag, int64_t nS, const float* pos, const float* vort,
                 const float* sigma, const int32_t* flag, float scale, float* u) {
	REC_TRY
	std::vector<VortexParticleData> vp;
	fill(vp, nS, pos, vort, sigma, flag);
	std::vector<Vec3> res;
	if (self) {
		KnVpAdvectSelf k(vp, scale);
		res = k.getRet();
	} else {
		std::vector<Node> nodes;
		for (int64_t i = 0; i < nT; i++) {
			nodes.push_back(Node(Vec3(tpos[3 * i], tpos[3 * i + 1], tpos[3 * i + 2])));
			nodes[i].flags = tflag[i];
		}
		KnVpAdvectMesh k(nodes, vp, scale);
		res = k.getRet();
	}
	for (size_t i = 0; i < res.size(); i++)
		for (int c = 0; c < 3; c++) u[3 * i + c] = res[i][c];
	REC_CATCH
}

/* VortexParticleSystem::advectSelf on a solver with time step dt; pos is updated in place */
int rec_advect_self(int64_t n, float* pos, const float* vort, const float* sigma, const int32_t* flag, float scale, float dt, int mode) {
	REC_TRY
	FluidSolver s(Vec3i(8, 8, 8), 3);
	s.mDt = dt;
	VortexParticleSystem sys(&s);
	fill(sys, n, pos, vort, sigma, flag);
	sys.advectSelf(scale, mode);
	for (int64_t i = 0; i < n; i++)
		for (int c = 0; c < 3; c++) pos[3 * i + c] = sys[i].pos[c];
	REC_CATCH
}

/* VortexParticleSystem::applyToMesh; nodes is updated in place */
int rec_apply_to_mesh(int64_t nT, float* nodes, const int32_t* nflags, int64_t nS, const float* pos, const float* vort, const float* sigma,
                      const int32_t* flag, float scale, float dt, int mode) {
	REC_TRY
	FluidSolver s(Vec3i(8, 8, 8), 3);
	s.mDt = dt;
	VortexParticleSystem sys(&s);
	fill(sys, nS, pos, vort, sigma, flag);
	Mesh mesh(&s);
	fill(mesh, nT, nodes, nflags);
	sys.applyToMesh(mesh, scale, mode);
	for (int64_t i = 0; i < nT; i++)
		for (int c = 0; c < 3; c++) nodes[3 * i + c] = mesh.nodes(i).pos[c];
	REC_CATCH
}

/* ---- VPseedK41: a stage per case, the calls of a case append to one system ---- */
int rec_seed_open(int sx, int sy, int sz, float dt) {
	REC_TRY
	g_sys.reset();
	g_solver.reset(new FluidSolver(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2));
	g_solver->mDt = dt;
	g_sys.reset(new VortexParticleSystem(g_solver.get()));
	REC_CATCH
}
/* kind 0: Box(p0 = a, p1 = b); kind 1: Sphere(center = a, radius = b[0]) */
int rec_seed_call(int kind, const float* a, const float* b, float strength, float sigma0, float sigma1, float probability, float N) {
	REC_TRY
	std::unique_ptr<Shape> sh = make_shape(g_solver.get(), kind, a, b);
	VPseedK41(*g_sys, sh.get(), strength, sigma0, sigma1, probability, N);
	REC_CATCH
}
int64_t rec_seed_size(void) { return g_sys ? (int64_t)g_sys->size() : -1; }
int rec_seed_read(int64_t cap, float* pos, float* vort, float* sigma, int32_t* flag) {
	REC_TRY
	read_system(*g_sys, cap, pos, vort, sigma, flag);
	REC_CATCH
}
int rec_seed_close(void) {
	REC_TRY
	g_sys.reset();
	g_solver.reset();
	REC_CATCH
}

int rec_density(int sx, int sy, int sz, const float* phi, float* density, float value, float sigma) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	LevelsetGrid p(&s);
	Grid<Real> d(&s);
	const IndexInt n = (IndexInt)sx * sy * sz;
	for (IndexInt i = 0; i < n; i++) {
		p[i] = phi[i];
		d[i] = density[i];
	}
	densityFromLevelset(p, d, value, sigma);
	for (IndexInt i = 0; i < n; i++) density[i] = d[i];
	REC_CATCH
}

int rec_mark_as_fixed(int64_t n, const float* pos, int32_t* flags, const float* p0, const float* p1, int exclusive) {
	REC_TRY
	FluidSolver s(Vec3i(8, 8, 8), 3);
	Mesh mesh(&s);
	fill(mesh, n, pos, flags);
	Box box(&s, Vec3::Invalid, Vec3(p0[0], p0[1], p0[2]), Vec3(p1[0], p1[1], p1[2]), Vec3::Invalid);
	markAsFixed(mesh, &box, exclusive != 0);
	for (int64_t i = 0; i < n; i++) flags[i] = mesh.nodes(i).flags;
	REC_CATCH
}

/* the loop: per step VPseedK41 in a sphere, advectSelf(scale, RK4), advectInGrid(RK4, deleteInObstacle), and after the last step a
 * compress().  flags [n], vel [3][n] (SoA); sizes[steps]: the system's size after each step (before the final compress) */
int rec_loop(int sx, int sy, int sz, float dt, int steps, const int32_t* flags, const float* vel, const float* centre, float radius,
             float strength, float sigma0, float sigma1, float probability, float N, float scale, int64_t* sizes, int64_t cap,
             int64_t* np_out, float* pos, float* vort, float* sigma, int32_t* flag) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), 3);
	s.mDt = dt;
	FlagGrid fl(&s);
	MACGrid v(&s);
	const IndexInt n = (IndexInt)sx * sy * sz;
	for (IndexInt i = 0; i < n; i++) {
		fl[i] = flags[i];
		v[i] = Vec3(vel[i], vel[n + i], vel[2 * n + i]);
	}
	VortexParticleSystem sys(&s);
	Sphere ball(&s, Vec3(centre[0], centre[1], centre[2]), radius, Vec3(1, 1, 1));
	for (int t = 0; t < steps; t++) {
		VPseedK41(sys, &ball, strength, sigma0, sigma1, probability, N);
		sys.advectSelf(scale, 2);
		sys.advectInGrid(fl, v, 2, true, true, false, nullptr, 0);
		sizes[t] = sys.size();
	}
	sys.doCompress(true);
	*np_out = read_system(sys, cap, pos, vort, sigma, flag);
	REC_CATCH
}

}  // extern "C"
