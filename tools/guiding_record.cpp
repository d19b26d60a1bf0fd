/*
 * tools/guiding_record.cpp -- the C++ half of the recorder of tests/golden/guiding.npz (tools/record_guiding.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid objects around
 * caller-owned arrays and calls the reference's own fluid-guiding functions, plus the main loops of tools/tests/test_1050_guiding2d.py
 * and scenes/guiding_3d02_high.py written against the reference's classes (same calls, same arguments, same order).  It is compiled
 * in a scratch directory together with the expanded plugin/fluidguiding.cpp (which oracle/ref.mk does not build) and linked against
 * oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled with is committed.
 *
 * Array conventions are those of include/manta_hip.h: MAC grids are SoA ([3][n]).
 */
#include "manta.h"
#include "grid.h"
#include "particle.h"
#include "shapes.h"
#include "noisefield.h"
#include "rcmatrix.h"
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace Manta {
// functions of plugin/fluidguiding.cpp (external linkage; no header declares them)
Matrix get1DGaussianBlurKernel(const int n, const int sigma);
void ADMM_precompute_Separable(int blurRadius);
extern Matrix gBlurKernel;
void precomputeQ(MACGrid& Q, const FlagGrid& flags, const MACGrid& velT_region, const MACGrid& velC, const Matrix& gBlurKernel, const Real sigma);
void precomputeInvA(MACGrid& invA, const Grid<Real>& weight, const Real sigma);
void prox_f(MACGrid& v, const FlagGrid& flags, const MACGrid& Q, const MACGrid& velC, const Real sigma, const MACGrid& invA);
Real getRNorm(const MACGrid& x, const MACGrid& z);
Real getEpsDual(const Real eps_abs, const Real eps_rel, const MACGrid& y);
void getSpiralVelocity(const FlagGrid& flags, MACGrid& vel, Real strength, bool with3D);
void setGradientYWeight(Grid<Real>& W, const int minY, const int maxY, const Real valAtMin, const Real valAtMax);
void PD_fluid_guiding(MACGrid& vel, MACGrid& velT, Grid<Real>& pressure, FlagGrid& flags, Grid<Real>& weight, int blurRadius, Real theta, Real tau,
                      Real sigma, Real epsRel, Real epsAbs, int maxIters, Grid<Real>* phi, Grid<Real>* perCellCorr, MACGrid* fractions, MACGrid* obvel,
                      Real gfClamp, Real cgMaxIterFac, Real cgAccuracy, int preconditioner, bool zeroPressureFixing, const Grid<Real>* curv,
                      const Real surfTens);
void releaseBlurPrecomp();
// other PYTHON() plugins (plain functions in the NOPYTHON packaging)
void solvePressure(MACGrid& vel, Grid<Real>& pressure, const FlagGrid& flags, Real cgAccuracy, const Grid<Real>* phi,
                   const Grid<Real>* perCellCorr, const MACGrid* fractions, const MACGrid* obvel, Real gfClamp, Real cgMaxIterFac,
                   bool precondition, int preconditioner, bool enforceCompatibility, bool useL2Norm, bool zeroPressureFixing,
                   const Grid<Real>* curv, const Real surfTens, Grid<Real>* retRhs);
void advectSemiLagrange(const FlagGrid* flags, const MACGrid* vel, GridBase* grid, int order, Real strength, int orderSpace, bool openBounds,
                        int boundaryWidth, int clampMode, int orderTrace);
void setWallBcs(const FlagGrid& flags, MACGrid& vel, const MACGrid* obvel, const MACGrid* fractions, const Grid<Real>* phiObs, int boundaryWidth);
void addBuoyancy(const FlagGrid& flags, const Grid<Real>& density, MACGrid& vel, Vec3 gravity, Real coefficient, bool scale);
void densityInflow(const FlagGrid& flags, Grid<Real>& density, const WaveletNoiseField& noise, Shape* shape, Real scale, Real sigma);
void setOpenBound(FlagGrid& flags, int bWidth, std::string openBound, int type);
void resetOutflow(FlagGrid& flags, Grid<Real>* phi, BasicParticleSystem* parts, Grid<Real>* real, Grid<int>* index, ParticleIndexSystem* indexSys);
void releaseMG(FluidSolver* solver);
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
void loadMac(MACGrid& g, const float* s, int64_t n) {
	for (int64_t i = 0; i < n; i++) g[i] = Vec3(s[i], s[n + i], s[2 * n + i]);
}
void storeMac(const MACGrid& g, float* s, int64_t n) {
	for (int64_t i = 0; i < n; i++) {
		s[i] = g[i].x;
		s[n + i] = g[i].y;
		s[2 * n + i] = g[i].z;
	}
}
// the iteration counts of a guiding call, from the reference's own debug lines (pressure.cpp:442, fluidguiding.cpp:352)
struct Capture {
	std::ostringstream buf;
	std::streambuf* old;
	int level;
	Capture() : old(std::cout.rdbuf(buf.rdbuf())), level(gDebugLevel) { gDebugLevel = 2; }
	~Capture() {
		std::cout.rdbuf(old);
		gDebugLevel = level;
	}
	std::vector<int> all(const char* key) {
		std::vector<int> r;
		const std::string s = buf.str();
		for (size_t p = s.find(key); p != std::string::npos; p = s.find(key, p + 1)) r.push_back(atoi(s.c_str() + p + strlen(key)));
		return r;
	}
};
// one guided step's counts appended to the outputs: pd[step], cg[...] with *ncg the running total
void guided(MACGrid& vel, MACGrid& velT, Grid<Real>& pressure, FlagGrid& flags, Grid<Real>& W, int blurRadius, Real theta, Real tau, Real sigma,
            Real epsRel, Real epsAbs, int maxIters, int preconditioner, bool zeroPressureFixing, int32_t* pd, int32_t* cg, int cg_cap, int32_t* ncg) {
	Capture c;
	PD_fluid_guiding(vel, velT, pressure, flags, W, blurRadius, theta, tau, sigma, epsRel, epsAbs, maxIters, nullptr, nullptr, nullptr, nullptr, 1e-04,
	                 1.5, 1e-3, preconditioner, zeroPressureFixing, nullptr, 0.);
	const std::vector<int> p = c.all("PD_fluid_guiding iterations:"), q = c.all("Iterations:");
	if (p.size() != 1) throw std::runtime_error("guided: no iteration line");
	*pd = p[0];
	if ((int)q.size() != p[0] + 1) throw std::runtime_error("guided: CG lines do not match the iteration count");
	for (int v : q) {
		if (*ncg >= cg_cap) throw std::runtime_error("guided: cg_cap too small");
		cg[(*ncg)++] = v;
	}
}
}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

int rec_weights(int radius, float* out) {
	REC_TRY
	const int n = 2 * radius + 1;
	Matrix G = get1DGaussianBlurKernel(n, n);
	for (int j = 0; j < n; j++) out[j] = G(0, j);
	REC_CATCH
}

int rec_spiral(int sx, int sy, int sz, float* vel, float strength, int with3D) {
	REC_TRY
	FluidSolver solver(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	const int64_t n = (int64_t)sx * sy * sz;
	FlagGrid fl(&solver);
	MACGrid v(&solver);
	loadMac(v, vel, n);
	getSpiralVelocity(fl, v, strength, with3D != 0);
	storeMac(v, vel, n);
	REC_CATCH
}

int rec_gradient(int sx, int sy, int sz, float* W, int minY, int maxY, float valAtMin, float valAtMax) {
	REC_TRY
	FluidSolver solver(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> w(&solver, W);
	setGradientYWeight(w, minY, maxY, valAtMin, valAtMax);
	REC_CATCH
}

/* one PD_fluid_guiding call on caller-owned grids (case c).  vel is updated, pressure written. */
int rec_guiding(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* velT, float* pressure, const float* weight, int blurRadius,
                float theta, float tau, float sigma, float epsRel, float epsAbs, int maxIters, int preconditioner, int32_t* pd, int32_t* cg, int cg_cap,
                int32_t* ncg) {
	REC_TRY
	FluidSolver solver(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	const int64_t n = (int64_t)sx * sy * sz;
	FlagGrid fl(&solver, const_cast<int32_t*>(flags));
	Grid<Real> p(&solver, pressure), w(&solver, const_cast<float*>(weight));
	MACGrid v(&solver), vT(&solver);
	loadMac(v, vel, n);
	loadMac(vT, velT, n);
	releaseBlurPrecomp();
	*ncg = 0;
	guided(v, vT, p, fl, w, blurRadius, theta, tau, sigma, epsRel, epsAbs, maxIters, preconditioner, false, pd, cg, cg_cap, ncg);
	releaseBlurPrecomp();
	storeMac(v, vel, n);
	REC_CATCH
}

/* the same call taken apart (the loop of fluidguiding.cpp:304-347 over the reference's own helper functions), `iters` iterations without
 * a stop test; per iteration: x, z before the solve, z after it, y ([iters][3][n] each) and rnorm, epsDual ([iters]) */
int rec_staged(int sx, int sy, int sz, const int32_t* flags, const float* vel, const float* velT, const float* weight, int blurRadius, float theta,
               float tau, float sigma, float epsRel, float epsAbs, int preconditioner, int iters, float* x_out, float* zpre_out, float* zpost_out,
               float* y_out, float* rnorm_out, float* eps_out, float* q_out, float* inva_out) {
	REC_TRY
	FluidSolver solver(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	const int64_t n = (int64_t)sx * sy * sz;
	FlagGrid fl(&solver, const_cast<int32_t*>(flags));
	Grid<Real> pressure(&solver), w(&solver, const_cast<float*>(weight));
	MACGrid velC(&solver), vT(&solver), x(&solver), y(&solver), z(&solver), x0(&solver), z0(&solver), Q(&solver), invA(&solver);
	loadMac(velC, vel, n);
	loadMac(vT, velT, n);
	releaseBlurPrecomp();
	ADMM_precompute_Separable(blurRadius);
	precomputeQ(Q, fl, vT, velC, gBlurKernel, sigma);
	precomputeInvA(invA, w, sigma);
	storeMac(Q, q_out, n);
	for (int64_t i = 0; i < n; i++) inva_out[i] = invA[i].x;
	for (int it = 0; it < iters; it++) {
		x0.copyFrom(x);
		x.multConst(1.0 / sigma);
		x.add(y);
		prox_f(x, fl, Q, velC, sigma, invA);
		x.multConst(-sigma);
		x.addScaled(y, sigma);
		x.add(x0);
		z0.copyFrom(z);
		z.addScaled(x, -tau);
		storeMac(x, x_out + 3 * n * it, n);
		storeMac(z, zpre_out + 3 * n * it, n);
		solvePressure(z, pressure, fl, 1e-3, nullptr, nullptr, nullptr, nullptr, 1e-04, 1.5, true, preconditioner, false, false, false, nullptr, 0., nullptr);
		storeMac(z, zpost_out + 3 * n * it, n);
		y.copyFrom(z);
		y.sub(z0);
		y.multConst(theta);
		y.add(z);
		storeMac(y, y_out + 3 * n * it, n);
		rnorm_out[it] = getRNorm(z, z0);
		eps_out[it] = getEpsDual(epsAbs, epsRel, z);
	}
	releaseBlurPrecomp();
	REC_CATCH
}

/* tools/tests/test_1050_guiding2d.py's main loop at res x res (2-D).  Shape::applyToGrid needs the Python argument store (NOPYTHON
 * build: errMsg), so the source is applied with the shape's own isInsideGrid. */
int rec_loop_2d(int res, int steps, int scale, int blurRadius, float theta, float tau, float sigma, float epsRel, float epsAbs, int maxIters,
                int preconditioner, int32_t* pd, int32_t* cg, int cg_cap, int32_t* ncg, float* vel_out, float* density_out, float* pressure_out) {
	REC_TRY
	const Vec3i gsi(res, res, 1);
	const Vec3 gs(res, res, 1);
	FluidSolver s(gsi, 2);
	s.mDt = 2.0 / scale;
	FlagGrid flags(&s);
	MACGrid vel(&s), velT(&s);
	Grid<Real> density(&s), pressure(&s), W(&s);
	flags.initDomain(1, "xXyYzZ", "      ", "      ", "      ", nullptr);
	flags.fillGrid();
	Cylinder source(&s, gs * Vec3(0.5, 0.3, 0.5), gs.y * 0.14, gs * Vec3(0, 0.04 * 1.5, 0));
	getSpiralVelocity(flags, velT, 1.5 * scale, false);
	setGradientYWeight(W, 0, res / 2, 1, 1);
	setGradientYWeight(W, res / 2, res, 5, 5);
	releaseBlurPrecomp();
	*ncg = 0;
	for (int t = 0; t < steps; t++) {
		resetOutflow(flags, nullptr, nullptr, &density, nullptr, nullptr);
		FOR_IJK(density) if (source.isInsideGrid(i, j, k)) density(i, j, k) = 1;
		advectSemiLagrange(&flags, &vel, &density, 2, 1.0, 1, false, -1, 1, 1);
		advectSemiLagrange(&flags, &vel, &vel, 2, 1.0, 1, false, -1, 1, 1);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		addBuoyancy(flags, density, vel, Vec3(0, 0.25 * scale * -1e-2, 0), 1.0, true);
		guided(vel, velT, pressure, flags, W, blurRadius, theta, tau, sigma, epsRel, epsAbs, maxIters, preconditioner, false, pd + t, cg, cg_cap, ncg);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		s.step();
	}
	releaseBlurPrecomp();
	const int64_t n = (int64_t)res * res;
	storeMac(vel, vel_out, n);
	for (int64_t i = 0; i < n; i++) {
		density_out[i] = density[i];
		pressure_out[i] = pressure[i];
	}
	REC_CATCH
}

/* scenes/guiding_3d02_high.py's main loop at res2 x 2 res2 x res2, the target velocity from getSpiralVelocity(with3D) in place of the
 * low-resolution files */
int rec_loop_3d(int res2, int steps, int factor, float timestep, int blurRadius, float wScalar, float theta, float tau, float sigma, float epsRel,
                float epsAbs, int maxIters, int preconditioner, int32_t* pd, int32_t* cg, int cg_cap, int32_t* ncg, float* vel_out, float* density_out,
                float* pressure_out) {
	REC_TRY
	const Vec3i gsi(res2, 2 * res2, res2);
	const Vec3 gs2(gsi.x, gsi.y, gsi.z);
	FluidSolver s2(gsi, 3);
	s2.mDt = timestep;
	FlagGrid flags(&s2);
	MACGrid vel(&s2), velT(&s2);
	Grid<Real> density(&s2), pressure(&s2), W(&s2);
	WaveletNoiseField noise(&s2, -1, 0);
	noise.mPosScale = Vec3(0);
	noise.mClamp = true;
	noise.mClampNeg = 0;
	noise.mClampPos = 1;
	noise.mValScale = 1;
	noise.mValOffset = 0.75;
	noise.mTimeAnim = 0.2;
	flags.initDomain(0, "xXyYzZ", "      ", "      ", "      ", nullptr);
	flags.fillGrid();
	setOpenBound(flags, 0, "yY", FlagGrid::TypeOutflow | FlagGrid::TypeEmpty);
	Cylinder source(&s2, gs2 * Vec3(0.5, 0.05, 0.5), res2 * 0.1, gs2 * Vec3(0, 0.02, 0));
	W.multConst(0);
	W.addConst(wScalar);
	releaseBlurPrecomp();
	*ncg = 0;
	for (int t = 0; t < steps; t++) {
		densityInflow(flags, density, noise, &source, 1, 0.5);
		advectSemiLagrange(&flags, &vel, &density, 2, 1.0, 1, false, -1, 2, 1);
		advectSemiLagrange(&flags, &vel, &vel, 2, 1.0, 1, false, -1, 2, 1);
		resetOutflow(flags, nullptr, nullptr, &density, nullptr, nullptr);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		addBuoyancy(flags, density, vel, Vec3(0, -1e-3 * factor, 0), 1.0, true);
		getSpiralVelocity(flags, velT, 1.0, true);
		velT.multConst(Vec3(factor));
		guided(vel, velT, pressure, flags, W, blurRadius, theta, tau, sigma, epsRel, epsAbs, maxIters, preconditioner, true, pd + t, cg, cg_cap, ncg);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		s2.step();
	}
	releaseBlurPrecomp();
	releaseMG(&s2);
	const int64_t n = (int64_t)gsi.x * gsi.y * gsi.z;
	storeMac(vel, vel_out, n);
	for (int64_t i = 0; i < n; i++) {
		density_out[i] = density[i];
		pressure_out[i] = pressure[i];
	}
	REC_CATCH
}

}  // extern "C"
