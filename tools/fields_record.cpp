/*
 * tools/fields_record.cpp -- the C++ half of the recorder of tests/golden/fields.npz (tools/record_fields.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid objects around
 * caller-owned arrays and calls the reference's own plugins.  plugin/fire.cpp and plugin/waves.cpp are not part of oracle/ref.mk's
 * library: the recorder's commands expand them with the reference's `prep` into a scratch directory, and this file takes them into
 * its own translation unit (the two includes below), because the right-hand-side kernel of cgSolveWE has no name outside its file.
 * The uv plugins, extrapolateSimpleFlags and initVortexVelocity are in the library.  It is compiled in a scratch directory and linked
 * against oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled with is committed.
 */
#include "plugin/fire.cpp"
#include "plugin/waves.cpp"

#include "manta.h"
#include "grid.h"
#include "shapes.h"
#include "levelset.h"
#include "particle.h"
#include <cmath>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <memory>
#include <vector>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
Real getUvWeight(Grid<Vec3>& uv);
void resetUvGrid(Grid<Vec3>& target, const Vec3* offset);
void updateUvWeight(Real resetTime, int index, int numUvs, Grid<Vec3>& uv, const Vec3* offset);
void extrapolateSimpleFlags(const FlagGrid& flags, GridBase* val, int distance, int flagFrom, int flagTo);
void initVortexVelocity(const Grid<Real>& phiObs, MACGrid& vel, const Vec3& center, const Real& radius);
void advectSemiLagrange(const FlagGrid* flags, const MACGrid* vel, GridBase* grid, int order, Real strength, int orderSpace, bool openBounds,
                        int boundaryWidth, int clampMode, int orderTrace);
void setWallBcs(const FlagGrid& flags, MACGrid& vel, const MACGrid* obvel, const MACGrid* fractions, const Grid<Real>* phiObs, int boundaryWidth);
void addBuoyancy(const FlagGrid& flags, const Grid<Real>& density, MACGrid& vel, Vec3 gravity, Real coefficient, bool scale);
void solvePressure(MACGrid& vel, Grid<Real>& pressure, const FlagGrid& flags, Real cgAccuracy, const Grid<Real>* phi,
                   const Grid<Real>* perCellCorr, const MACGrid* fractions, const MACGrid* obvel, Real gfClamp, Real cgMaxIterFac,
                   bool precondition, int preconditioner, bool enforceCompatibility, bool useL2Norm, bool zeroPressureFixing,
                   const Grid<Real>* curv, const Real surfTens, Grid<Real>* retRhs);
void updateFractions(const FlagGrid& flags, const Grid<Real>& phiObs, MACGrid& fractions, const int& boundaryWidth, const Real fracThreshold);
void setObstacleFlags(FlagGrid& flags, const Grid<Real>& phiObs, const MACGrid* fractions, const Grid<Real>* phiOut, const Grid<Real>* phiIn,
                      int boundaryWidth);
void extrapolateMACSimple(FlagGrid& flags, MACGrid& vel, int distance, LevelsetGrid* phiObs, bool intoObs);
void setOpenBound(FlagGrid& flags, int bWidth, std::string openBound, int type);
void resetOutflow(FlagGrid& flags, Grid<Real>* phi, BasicParticleSystem* parts, Grid<Real>* real, Grid<int>* index, ParticleIndexSystem* indexSys);
void vorticityConfinement(MACGrid& vel, const FlagGrid& flags, Real strength, const Grid<Real>* strengthCell);
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
void load(Grid<int>& g, const int32_t* a) { for (IndexInt i = 0; i < cells(g); i++) g[i] = a[i]; }
void store(const Grid<int>& g, int32_t* a) { for (IndexInt i = 0; i < cells(g); i++) a[i] = g[i]; }
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

// the iteration count of the last solve, from the reference's own debug line (`<what>` is the text in front of the number)
struct Capture {
	std::ostringstream buf;
	std::streambuf* old;
	int level;
	Capture(int lvl) : old(std::cout.rdbuf(buf.rdbuf())), level(gDebugLevel) { gDebugLevel = lvl; }
	~Capture() {
		std::cout.rdbuf(old);
		gDebugLevel = level;
	}
	int iterations(const char* what) {
		const std::string s = buf.str();
		const size_t p = s.rfind(what);
		return p == std::string::npos ? -1 : atoi(s.c_str() + p + strlen(what));
	}
};

struct Opt {
	Grid<Real> g;
	bool on;
	Opt(FluidSolver* s, float* a) : g(s), on(a != nullptr) {
		if (on) load(g, a);
	}
	Grid<Real>* ptr() { return on ? &g : nullptr; }
	void out(float* a) {
		if (on) store(g, a);
	}
};

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* red / green / blue / heat may each be NULL; par = burningRate, flameSmoke, ignitionTemp, maxTemp, colour x y z */
int rec_process_burn(int sx, int sy, int sz, float dt, float* fuel, float* density, float* react, float* red, float* green, float* blue,
                     float* heat, const float* par) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	s.mDt = dt;
	Grid<Real> gf(&s), gd(&s), gr(&s);
	load(gf, fuel); load(gd, density); load(gr, react);
	Opt r(&s, red), g(&s, green), b(&s, blue), h(&s, heat);
	processBurn(gf, gd, gr, r.ptr(), g.ptr(), b.ptr(), h.ptr(), par[0], par[1], par[2], par[3], Vec3(par[4], par[5], par[6]));
	store(gf, fuel); store(gd, density); store(gr, react);
	r.out(red); g.out(green); b.out(blue); h.out(heat);
	REC_CATCH
}

int rec_update_flame(int sx, int sy, int sz, const float* react, float* flame) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> gr(&s), gf(&s);
	load(gr, react); load(gf, flame);
	updateFlame(gr, gf);
	store(gf, flame);
	REC_CATCH
}

int rec_sec_deriv(int sx, int sy, int sz, const float* v, float* curv) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> gv(&s), gc(&s);
	load(gv, v); load(gc, curv);
	calcSecDeriv2d(gv, gc);
	store(gc, curv);
	REC_CATCH
}

/* *sum = totalSum(h); then h = normalizeSumTo(h, target) */
int rec_sum_normalize(int sx, int sy, int sz, float* h, float target, float* sum) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> g(&s);
	load(g, h);
	*sum = totalSum(g);
	normalizeSumTo(g, target);
	store(g, h);
	REC_CATCH
}

/* the matrix and right-hand side of cgSolveWE, waves.cpp:107-126, for the scale factor sc the caller computed: the reference's
 * MakeLaplaceMatrix and MakeRhsWE kernels; the element-wise scaling between them is a loop inside cgSolveWE with no name, done here
 * with the grids' own multConst / addConst (an fp32 `+ 1` equals the loop's double sum rounded once) */
int rec_wave_system(int sx, int sy, int sz, float sc, int crankNic, const int32_t* flags, const float* ut, const float* utm1, float* A0, float* Ai,
                    float* Aj, float* Ak, float* rhs) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid f(&s);
	Grid<Real> gu(&s), gm(&s), a0(&s), ai(&s), aj(&s), ak(&s), r(&s);
	load(f, flags); load(gu, ut); load(gm, utm1);
	MakeLaplaceMatrix(f, a0, ai, aj, ak);
	ai.multConst(sc); aj.multConst(sc); ak.multConst(sc);
	a0.multConst(sc);
	a0.addConst(1);
	MakeRhsWE(f, r, gu, gm, sc, crankNic != 0);
	store(a0, A0); store(ai, Ai); store(aj, Aj); store(ak, Ak); store(r, rhs);
	REC_CATCH
}

int rec_cg_solve_we(int sx, int sy, int sz, float dt, const int32_t* flags, float* ut, float* utm1, float* out, int crankNic, float cSqr,
                    float cgMaxIterFac, float cgAccuracy, int* iterations) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	s.mDt = dt;
	FlagGrid f(&s);
	Grid<Real> gu(&s), gm(&s), go(&s);
	load(f, flags); load(gu, ut); load(gm, utm1); load(go, out);
	{
		Capture cap(1);
		cgSolveWE(f, gu, gm, go, crankNic != 0, cSqr, cgMaxIterFac, cgAccuracy);
		*iterations = cap.iterations("cgSolveWaveEq iterations:");
	}
	store(gu, ut); store(gm, utm1); store(go, out);
	REC_CATCH
}

int rec_reset_uv(int sx, int sy, int sz, float* uv, const float* offset) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Vec3> g(&s);
	load(g, uv);
	Vec3 off;
	if (offset) off = Vec3(offset[0], offset[1], offset[2]);
	resetUvGrid(g, offset ? &off : nullptr);
	store(g, uv);
	REC_CATCH
}

int rec_update_uv_weight(int sx, int sy, int sz, float t, float dt, float resetTime, int index, int numUvs, float* uv, const float* offset,
                         float* weight) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	s.mDt = dt;
	s.mTimeTotal = t;
	Grid<Vec3> g(&s);
	load(g, uv);
	Vec3 off;
	if (offset) off = Vec3(offset[0], offset[1], offset[2]);
	updateUvWeight(resetTime, index, numUvs, g, offset ? &off : nullptr);
	*weight = getUvWeight(g);
	store(g, uv);
	REC_CATCH
}

/* vtype 0: Grid<Real>, 1: Grid<int>, 2: Grid<Vec3>, 3: FlagGrid */
int rec_extrapolate(int sx, int sy, int sz, const int32_t* flags, void* val, int vtype, int distance, int flagFrom, int flagTo) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid f(&s);
	load(f, flags);
	if (vtype == 0) {
		Grid<Real> g(&s);
		load(g, (float*)val);
		extrapolateSimpleFlags(f, &g, distance, flagFrom, flagTo);
		store(g, (float*)val);
	} else if (vtype == 1) {
		Grid<int> g(&s);
		load(g, (int32_t*)val);
		extrapolateSimpleFlags(f, &g, distance, flagFrom, flagTo);
		store(g, (int32_t*)val);
	} else if (vtype == 2) {
		Grid<Vec3> g(&s);
		load(g, (float*)val);
		extrapolateSimpleFlags(f, &g, distance, flagFrom, flagTo);
		store(g, (float*)val);
	} else {
		FlagGrid g(&s);
		load(g, (int32_t*)val);
		extrapolateSimpleFlags(f, &g, distance, flagFrom, flagTo);
		store(g, (int32_t*)val);
	}
	REC_CATCH
}

int rec_vortex(int sx, int sy, int sz, const float* phiObs, float* vel, const float* center, float radius) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> p(&s);
	MACGrid v(&s);
	load(p, phiObs); load(v, vel);
	initVortexVelocity(p, v, Vec3(center[0], center[1], center[2]), radius);
	store(v, vel);
	REC_CATCH
}

/* ---- the four loops of tests/test_gpu_fields.py, written against the reference's classes ---- */

/* tools/tests/test_1030_waveeq.py's loop: explicit steps, implicit ones after step `switchAt`; h0 is the caller's initial height,
 * velFactor the Real the script's `cSqr * s.timestep` converts to.  iterations[t] = -1 for an explicit step. */
int rec_loop_wave(int sx, int sy, int steps, int switchAt, float dt, float cSqr, float velFactor, const float* h0, float* mass, int* iterations,
                  float* hOut, float* velOut) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, 1), 2);
	s.mDt = dt;
	Grid<Real> h(&s), hprev(&s), hnew(&s), curv(&s), vel(&s);
	FlagGrid flags(&s);
	flags.initDomain();
	flags.fillGrid();
	load(h, h0);
	hprev.copyFrom(h);
	bool implicit = false;
	for (int t = 0; t < steps; t++) {
		const Real m = totalSum(h);
		mass[t] = m;
		iterations[t] = -1;
		if (implicit) {
			Capture cap(1);
			cgSolveWE(flags, h, hprev, hnew, false, cSqr, 1.5, 1e-5);
			iterations[t] = cap.iterations("cgSolveWaveEq iterations:");
		} else {
			calcSecDeriv2d(h, curv);
			vel.addScaled(curv, velFactor);
			h.addScaled(vel, s.mDt);
			if (t >= switchAt) implicit = true;
		}
		normalizeSumTo(h, m);
		s.step();
	}
	store(h, hOut); store(vel, velOut);
	REC_CATCH
}

/* tools/tests/test_1020_uvs.py's main loop on the caller's velocity: uvOut = [numUvs][3][n], weights = [steps][numUvs] */
int rec_loop_uv(int sx, int sy, int steps, int numUvs, float dt, float resetTime, const float* vel, float* uvOut, float* weights) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, 1), 2);
	s.mDt = dt;
	FlagGrid flags(&s);
	flags.initDomain();
	flags.fillGrid();
	MACGrid v(&s);
	load(v, vel);
	std::vector<std::unique_ptr<Grid<Vec3>>> uv;
	for (int i = 0; i < numUvs; i++) {
		uv.emplace_back(new Grid<Vec3>(&s));
		resetUvGrid(*uv[i], nullptr);
	}
	for (int t = 0; t < steps; t++) {
		for (int i = 0; i < numUvs; i++) {
			advectSemiLagrange(&flags, &v, uv[i].get(), 1, 1.0, 1, false, -1, 2, 1);
			updateUvWeight(resetTime, i, numUvs, *uv[i], nullptr);
			weights[t * numUvs + i] = getUvWeight(*uv[i]);
		}
		s.step();
	}
	const IndexInt n = cells(flags);
	for (int i = 0; i < numUvs; i++) store(*uv[i], uvOut + 3 * n * i);
	REC_CATCH
}

/* tools/tests/test_1040_secOrderBnd.py (new_BC) at res x res */
int rec_loop_bnd(int res, int steps, float* fracOut, float* velOut, int* iterations) {
	REC_TRY
	FluidSolver s(Vec3i(res, res, 1), 2);
	s.mDt = 1;
	FlagGrid flags(&s);
	MACGrid vel(&s), fractions(&s);
	Grid<Real> pressure(&s), density(&s);
	flags.initDomain();
	const Vec3 center = Vec3(res, res, 1) * Vec3(0.5, 0.5, 0.5);
	const Real radius = res * 0.4;
	Sphere sphere(&s, center, radius);
	LevelsetGrid phiObs(&s);
	phiObs.copyFrom(sphere.computeLevelset());
	phiObs.multConst(-1);
	initVortexVelocity(phiObs, vel, center, radius);
	updateFractions(flags, phiObs, fractions, 0, 0.01);
	setObstacleFlags(flags, phiObs, &fractions, nullptr, nullptr, 1);
	flags.fillGrid();
	for (int t = 0; t < steps; t++) {
		advectSemiLagrange(&flags, &vel, &density, 2, 1.0, 1, false, -1, 1, 1);
		advectSemiLagrange(&flags, &vel, &vel, 2, 1.0, 1, false, -1, 1, 1);
		setWallBcs(flags, vel, nullptr, &fractions, &phiObs, 0);
		extrapolateMACSimple(flags, vel, 1, nullptr, false);
		{
			Capture cap(2);
			solvePressure(vel, pressure, flags, 1e-3, nullptr, nullptr, &fractions, nullptr, 1e-4, 1.5, true, 1, false, false, false, nullptr, 0., nullptr);
			iterations[t] = cap.iterations("Iterations:");
		}
		setWallBcs(flags, vel, nullptr, &fractions, &phiObs, 0);
		extrapolateMACSimple(flags, vel, 1, nullptr, false);
		s.step();
	}
	store(fractions, fracOut); store(vel, velOut);
	REC_CATCH
}

/* scenes/fire.py's loop at res^3 with its adaptive time step and open y bounds.  The four densityInflow calls are replaced by copies:
 * where mask != 0, density / heat / fuel / react take src[0..3].  par = dt0, frameLength, timestepMin, timestepMax, cfl, the y components of
 * the two buoyancy vectors, vortGlobal, vortFlames.  grids = density, heat, fuel, react, flame, pressure, vel x y z (9 planes).
 * powfCells = {cells in which powf(x, 0.5f) != sqrtf(x) over all processBurn calls, over all updateFlame calls}. */
int rec_loop_fire(int res, int steps, const float* par, const int32_t* mask, const float* src, float* dts, int* iterations, float* grids,
                  int64_t* powfCells) {
	REC_TRY
	FluidSolver s(Vec3i(res, res, res), 3);
	s.mFrameLength = par[1];
	s.mDtMin = par[2];
	s.mDtMax = par[3];
	s.mCflCond = par[4];
	s.mDt = par[0];
	FlagGrid flags(&s);
	MACGrid vel(&s);
	Grid<Real> density(&s), react(&s), fuel(&s), heat(&s), flame(&s), pressure(&s);
	flags.initDomain(1);
	flags.fillGrid();
	setOpenBound(flags, 1, "yY", FlagGrid::TypeOutflow | FlagGrid::TypeEmpty);
	const IndexInt n = cells(flags);
	Grid<Real>* into[4] = {&density, &heat, &fuel, &react};
	powfCells[0] = powfCells[1] = 0;
	auto interior = [&](IndexInt idx) {
		const int i = idx % res, j = (idx / res) % res, k = idx / ((IndexInt)res * res);
		return i >= 1 && i < res - 1 && j >= 1 && j < res - 1 && k >= 1 && k < res - 1;
	};
	for (int t = 0; t < steps; t++) {
		s.adaptTimestep(vel.getMax());
		dts[t] = s.mDt;
		for (int q = 0; q < 4; q++)
			for (IndexInt i = 0; i < n; i++)
				if (mask[i]) (*into[q])[i] = src[q * n + i];
		Grid<Real> fuel0(&s);
		fuel0.copyFrom(fuel);
		processBurn(fuel, density, react, nullptr, nullptr, nullptr, &heat, 0.75f, 1.0f, 1.25f, 1.75f, Vec3(0.7f, 0.7f, 0.7f));
		for (IndexInt i = 0; i < n; i++)
			if (interior(i) && fuel0[i] > 1e-6f && powf(react[i], 0.5f) != sqrtf(react[i]) && react[i] > 0) powfCells[0]++;
		advectSemiLagrange(&flags, &vel, &density, 2, 1.0, 1, false, -1, 2, 1);
		advectSemiLagrange(&flags, &vel, &heat, 2, 1.0, 1, false, -1, 2, 1);
		advectSemiLagrange(&flags, &vel, &fuel, 2, 1.0, 1, false, -1, 2, 1);
		advectSemiLagrange(&flags, &vel, &react, 2, 1.0, 1, false, -1, 2, 1);
		advectSemiLagrange(&flags, &vel, &vel, 2, 1.0, 1, false, -1, 2, 1);
		resetOutflow(flags, nullptr, nullptr, &density, nullptr, nullptr);
		flame.copyFrom(fuel);
		flame.multConst(par[8]);
		vorticityConfinement(vel, flags, par[7], &flame);
		addBuoyancy(flags, density, vel, Vec3(0, par[5], 0), 1., true);
		addBuoyancy(flags, heat, vel, Vec3(0, par[6], 0), 1., true);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		{
			Capture cap(2);
			solvePressure(vel, pressure, flags, 1e-3, nullptr, nullptr, nullptr, nullptr, 1e-4, 1.5, true, 1, false, false, false, nullptr, 0., nullptr);
			iterations[t] = cap.iterations("Iterations:");
		}
		for (IndexInt i = 0; i < n; i++)
			if (interior(i) && react[i] > 0 && powf(react[i], 0.5f) != sqrtf(react[i])) powfCells[1]++;
		updateFlame(react, flame);
		s.step();
	}
	Grid<Real>* outs[6] = {&density, &heat, &fuel, &react, &flame, &pressure};
	for (int q = 0; q < 6; q++) store(*outs[q], grids + q * n);
	store(vel, grids + 6 * n);
	REC_CATCH
}

}  // extern "C"
