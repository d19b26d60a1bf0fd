/*
 * tools/turbulence_record.cpp -- the C++ half of the recorder of tests/golden/turbulence.npz (tools/record_turbulence.py is the other
 * half; its header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid /
 * TurbulenceParticleSystem objects around caller-owned arrays and calls the reference's own k-epsilon plugins (plugin/kepsilon.cpp is
 * not part of oracle/ref.mk's library: the recorder's commands expand it with the reference's `prep` in a scratch directory and compile
 * it next to this file), the diagnostics of plugin/waveletturbulence.cpp and the turbulence particle system (both in the library), plus
 * the loop of tools/tests/test_2025_turb.py written against the reference's classes.  It is compiled in a scratch directory and linked
 * against oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled with is committed.
 */
#include "manta.h"
#include "grid.h"
#include "particle.h"
#include "shapes.h"
#include "noisefield.h"
#include "turbulencepart.h"
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void KEpsilonComputeProduction(const MACGrid& vel, Grid<Real>& k, Grid<Real>& eps, Grid<Real>& prod, Grid<Real>& nuT, Grid<Real>* strain, Real pscale);
void KEpsilonSources(Grid<Real>& k, Grid<Real>& eps, Grid<Real>& prod);
void KEpsilonBcs(const FlagGrid& flags, Grid<Real>& k, Grid<Real>& eps, Real intensity, Real nu, bool fillArea);
void KEpsilonGradientDiffusion(Grid<Real>& k, Grid<Real>& eps, Grid<Real>& nuT, Real sigmaU, MACGrid* vel);
void computeVorticity(const MACGrid& vel, Grid<Vec3>& vorticity, Grid<Real>* norm);
void computeStrainRateMag(const MACGrid& vel, Grid<Real>& mag);
void getCurl(const MACGrid& vel, Grid<Real>& vort, int comp);
void advectSemiLagrange(const FlagGrid* flags, const MACGrid* vel, GridBase* grid, int order, Real strength, int orderSpace, bool openBounds,
                        int boundaryWidth, int clampMode, int orderTrace);
void setWallBcs(const FlagGrid& flags, MACGrid& vel, const MACGrid* obvel, const MACGrid* fractions, const Grid<Real>* phiObs, int boundaryWidth);
void setInflowBcs(MACGrid& vel, std::string dir, Vec3 value);
void solvePressure(MACGrid& vel, Grid<Real>& pressure, const FlagGrid& flags, Real cgAccuracy, const Grid<Real>* phi,
                   const Grid<Real>* perCellCorr, const MACGrid* fractions, const MACGrid* obvel, Real gfClamp, Real cgMaxIterFac,
                   bool precondition, int preconditioner, bool enforceCompatibility, bool useL2Norm, bool zeroPressureFixing,
                   const Grid<Real>* curv, const Real surfTens, Grid<Real>* retRhs);
extern int gDebugLevel;
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

IndexInt cells(const GridBase& g) { return g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ(); }
void load(Grid<Real>& g, const float* a) { for (IndexInt i = 0; i < cells(g); i++) g[i] = a[i]; }
void store(const Grid<Real>& g, float* a) { for (IndexInt i = 0; i < cells(g); i++) a[i] = g[i]; }
void load(FlagGrid& g, const int32_t* a) { for (IndexInt i = 0; i < cells(g); i++) g[i] = a[i]; }
// Vec3 grids cross as SoA [3][n]
void load(Grid<Vec3>& g, const float* a) {
	const IndexInt n = cells(g);
	for (IndexInt i = 0; i < n; i++) g[i] = Vec3(a[i], a[n + i], a[2 * n + i]);
}
void store(const Grid<Vec3>& g, float* a) {
	const IndexInt n = cells(g);
	for (IndexInt i = 0; i < n; i++) {
		a[i] = g[i].x;
		a[n + i] = g[i].y;
		a[2 * n + i] = g[i].z;
	}
}

// the iteration count of the last solve, from the reference's own debug line (pressure.cpp:442)
struct Capture {
	std::ostringstream buf;
	std::streambuf* old;
	int level;
	Capture() : old(std::cout.rdbuf(buf.rdbuf())), level(gDebugLevel) { gDebugLevel = 2; }
	~Capture() {
		std::cout.rdbuf(old);
		gDebugLevel = level;
	}
	int iterations() {
		const std::string s = buf.str();
		const size_t p = s.rfind("Iterations:");
		return p == std::string::npos ? -1 : atoi(s.c_str() + p + 11);
	}
};

// one solver with its grids, noise field and turbulence particle system: the particle cases of the fixture run on it, one after the
// other, because seed()'s random stream and synthesize()'s clock and inflow offset are statics of the reference
struct Stage {
	FluidSolver s;
	FlagGrid flags;
	MACGrid vel;
	Grid<Real> k;
	WaveletNoiseField noise;
	TurbulenceParticleSystem sys;
	Stage(int sx, int sy, int sz, float dt) : s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2), flags(&s), vel(&s), k(&s), noise(&s, -1, 0), sys(&s, noise) { s.mDt = dt; }
};
std::unique_ptr<Stage> g_stage;

void read_system(TurbulenceParticleSystem& sys, int64_t cap, float* pos, float* color, float* tex0, float* tex1, int32_t* flag) {
	const int64_t n = sys.size();
	if (n > cap) throw std::runtime_error("turbulence_record: capacity too small");
	for (int64_t i = 0; i < n; i++) {
		const TurbulenceParticleData& p = sys[i];
		for (int c = 0; c < 3; c++) {
			pos[c * cap + i] = p.pos[c];
			color[c * cap + i] = p.color[c];
			tex0[c * cap + i] = p.tex0[c];
			tex1[c * cap + i] = p.tex1[c];
		}
		flag[i] = p.flag;
	}
}

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* strain may be NULL */
int rec_production(int sx, int sy, int sz, const float* vel, float* k, float* eps, float* prod, float* nuT, float* strain, float pscale) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	MACGrid v(&s);
	Grid<Real> gk(&s), ge(&s), gp(&s), gn(&s), gs(&s);
	load(v, vel); load(gk, k); load(ge, eps); load(gp, prod); load(gn, nuT);
	if (strain) load(gs, strain);
	KEpsilonComputeProduction(v, gk, ge, gp, gn, strain ? &gs : nullptr, pscale);
	store(gk, k); store(ge, eps); store(gp, prod); store(gn, nuT);
	if (strain) store(gs, strain);
	REC_CATCH
}

int rec_sources(int sx, int sy, int sz, float dt, float* k, float* eps, const float* prod) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	s.mDt = dt;
	Grid<Real> gk(&s), ge(&s), gp(&s);
	load(gk, k); load(ge, eps); load(gp, prod);
	KEpsilonSources(gk, ge, gp);
	store(gk, k); store(ge, eps);
	REC_CATCH
}

int rec_bcs(int sx, int sy, int sz, const int32_t* flags, float* k, float* eps, float intensity, float nu, int fillArea) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid fl(&s);
	Grid<Real> gk(&s), ge(&s);
	load(fl, flags); load(gk, k); load(ge, eps);
	KEpsilonBcs(fl, gk, ge, intensity, nu, fillArea != 0);
	store(gk, k); store(ge, eps);
	REC_CATCH
}

/* `calls` calls in a row; vel may be NULL */
int rec_graddiff(int sx, int sy, int sz, float dt, int calls, float* k, float* eps, const float* nuT, float sigmaU, float* vel) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	s.mDt = dt;
	Grid<Real> gk(&s), ge(&s), gn(&s);
	MACGrid v(&s);
	load(gk, k); load(ge, eps); load(gn, nuT);
	if (vel) load(v, vel);
	for (int c = 0; c < calls; c++) KEpsilonGradientDiffusion(gk, ge, gn, sigmaU, vel ? &v : nullptr);
	store(gk, k); store(ge, eps);
	if (vel) store(v, vel);
	REC_CATCH
}

/* mag, vort [3][n] (pre-filled by the caller), norm, curl [3][n]: getCurl's three components */
int rec_diagnostics(int sx, int sy, int sz, const float* vel, float* mag, float* vort, float* norm, float* curl) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	MACGrid v(&s);
	Grid<Real> gm(&s), gn(&s), gc(&s);
	Grid<Vec3> gv(&s);
	const IndexInt n = cells(gm);
	load(v, vel); load(gm, mag); load(gv, vort); load(gn, norm);
	computeStrainRateMag(v, gm);
	computeVorticity(v, gv, &gn);
	store(gm, mag); store(gv, vort); store(gn, norm);
	for (int c = 0; c < 3; c++) {
		for (IndexInt i = 0; i < n; i++) gc[i] = 123.f;
		getCurl(v, gc, c);
		store(gc, curl + c * n);
	}
	REC_CATCH
}

/* ---- the particle stage ---- */
int rec_stage_open(int sx, int sy, int sz, float dt, const int32_t* flags, const float* vel, const float* k) {
	REC_TRY
	g_stage.reset();
	g_stage.reset(new Stage(sx, sy, sz, dt));
	load(g_stage->flags, flags); load(g_stage->vel, vel); load(g_stage->k, k);
	REC_CATCH
}
int rec_stage_close(void) {
	REC_TRY
	g_stage.reset();
	REC_CATCH
}
/* kind 0: Box(center = a, size = b); kind 1: Sphere(center = a, radius = b[0]) */
int rec_stage_seed(int kind, const float* a, const float* b, int num) {
	REC_TRY
	Stage& S = *g_stage;
	if (kind == 0) {
		Box box(&S.s, Vec3(a[0], a[1], a[2]), Vec3::Invalid, Vec3::Invalid, Vec3(b[0], b[1], b[2]));
		S.sys.seed(&box, num);
	} else {
		Sphere sp(&S.s, Vec3(a[0], a[1], a[2]), b[0], Vec3(1, 1, 1));
		S.sys.seed(&sp, num);
	}
	REC_CATCH
}
int rec_stage_advect(void) {
	REC_TRY
	Stage& S = *g_stage;
	S.sys.advectInGrid(S.flags, S.vel, 2 /* IntRK4 */, true, true, false, nullptr, 0);
	REC_CATCH
}
int rec_stage_synthesize(int octaves, float switchLength, float L0, float scale, const float* bias) {
	REC_TRY
	Stage& S = *g_stage;
	S.sys.synthesize(S.flags, S.k, octaves, switchLength, L0, scale, Vec3(bias[0], bias[1], bias[2]));
	REC_CATCH
}
int rec_stage_delete(void) {
	REC_TRY
	g_stage->sys.deleteInObstacle(g_stage->flags);
	REC_CATCH
}
int rec_stage_move(int64_t i, const float* p) {
	REC_TRY
	if (i < 0 || i >= g_stage->sys.size()) throw std::runtime_error("rec_stage_move: no such particle");
	g_stage->sys[i].pos = Vec3(p[0], p[1], p[2]);
	REC_CATCH
}
int rec_stage_clear(void) {
	REC_TRY
	g_stage->sys.clear();
	REC_CATCH
}
int64_t rec_stage_size(void) { return g_stage ? (int64_t)g_stage->sys.size() : -1; }
int rec_stage_read(int64_t cap, float* pos, float* color, float* tex0, float* tex1, int32_t* flag) {
	REC_TRY
	read_system(g_stage->sys, cap, pos, color, tex0, tex1, flag);
	REC_CATCH
}

/* the loop of tools/tests/test_2025_turb.py at gridSize (res, res / 2, res / 2); obstacleGradient / obstacleLevelset / createMesh are
 * left out (their results are not used in the loop).  per_step [steps][2]: particles after deleteInObstacle, CG iterations.
 * grids: k, eps, prod, nuT, strain, pressure [n] each, then vel [3][n].  The particle system is read at the end. */
int rec_loop(int res, int steps, float dt, int64_t* per_step, float* grids, int64_t cap, int64_t* np_out, float* pos, float* color, float* tex0,
             float* tex1, int32_t* flag, int64_t* obstacle_cells) {
	REC_TRY
	const Vec3i gsi(res, res / 2, res / 2);
	const Vec3 gs(res, res / 2, res / 2);
	FluidSolver s(gsi, 3);
	s.mDt = dt;
	const Vec3 velInflow(0.52, 0, 0);
	FlagGrid flags(&s);
	Grid<Real> pressure(&s), k(&s), eps(&s), prod(&s), nuT(&s), strain(&s);
	MACGrid vel(&s);
	WaveletNoiseField noise(&s, -1, 0);
	TurbulenceParticleSystem turb(&s, noise);
	flags.initDomain(0, "xXyYzZ", "      ", "      ", "      ", nullptr);
	flags.fillGrid();
	int64_t obs_cells = 0;
	for (int i = 0; i < 4; i++)
		for (int j = 0; j < 4; j++) {
			Sphere obs(&s, gs * Vec3(0.2, (i + 1) / 5.0, (j + 1) / 5.0), res * 0.025, Vec3(1, 1, 1));
			// Shape::applyToGrid(grid = flags, value = FlagObstacle) is ApplyShapeToGrid (shapes.cpp:41-47); the NOPYTHON packaging has
			// no `value` argument, so the kernel's body stands here
			FOR_IJK(flags) {
				if (obs.isInsideGrid(i, j, k)) {
					if (flags(i, j, k) != FlagGrid::TypeObstacle) obs_cells++;
					flags(i, j, k) = FlagGrid::TypeObstacle;
				}
			}
		}
	*obstacle_cells = obs_cells;
	Box box(&s, gs * Vec3(0.05, 0.43, 0.6), Vec3::Invalid, Vec3::Invalid, gs * Vec3(0.02, 0.005, 0.07));
	const Real L0 = 0.01, mult = 0.1, intensity = 0.1, nu = 0.1, prodMult = 2.5;
	KEpsilonBcs(flags, k, eps, intensity, nu, true);
	for (int t = 0; t < steps; t++) {
		turb.seed(&box, 500);
		turb.advectInGrid(flags, vel, 2 /* IntRK4 */, true, true, false, nullptr, 0);
		turb.synthesize(flags, k, 1, 5, L0, mult, velInflow);
		turb.deleteInObstacle(flags);
		per_step[2 * t] = turb.size();
		KEpsilonBcs(flags, k, eps, intensity, nu, false);
		advectSemiLagrange(&flags, &vel, &k, 1, 1.0, 1, false, -1, 2, 1);
		advectSemiLagrange(&flags, &vel, &eps, 1, 1.0, 1, false, -1, 2, 1);
		KEpsilonBcs(flags, k, eps, intensity, nu, false);
		KEpsilonComputeProduction(vel, k, eps, prod, nuT, &strain, prodMult);
		KEpsilonSources(k, eps, prod);
		KEpsilonGradientDiffusion(k, eps, nuT, 10.0, &vel);
		advectSemiLagrange(&flags, &vel, &vel, 2, 1.0, 1, false, -1, 1, 1);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		setInflowBcs(vel, "xXyYzZ", velInflow);
		{
			Capture c;
			solvePressure(vel, pressure, flags, 1e-3, nullptr, nullptr, nullptr, nullptr, 1e-04, 0.5, true, 1, false, false, false, nullptr, 0., nullptr);
			per_step[2 * t + 1] = c.iterations();
		}
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		setInflowBcs(vel, "xXyYzZ", velInflow);
		s.step();
	}
	const IndexInt n = cells(k);
	store(k, grids); store(eps, grids + n); store(prod, grids + 2 * n); store(nuT, grids + 3 * n); store(strain, grids + 4 * n);
	store(pressure, grids + 5 * n); store(vel, grids + 6 * n);
	*np_out = turb.size();
	read_system(turb, cap, pos, color, tex0, tex1, flag);
	REC_CATCH
}

}  // extern "C"
