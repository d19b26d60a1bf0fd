/*
 * tools/datagen_record.cpp -- the C++ half of the recorder of tests/golden/datagen.npz (tools/record_datagen.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid objects around
 * caller-owned arrays and calls the reference's own blurRealGrid, blurMacGrid, calcCenterOfMass, projectPpmFull, getLaplacian and
 * getCurvature, all of which are in the library of oracle/ref.mk (plugin/initplugins.cpp, plugin/flip.cpp, util/simpleimage.cpp).
 * Linked against oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled with is committed.
 */
#include "manta.h"
#include "grid.h"
#include "levelset.h"
#include "noisefield.h"
#include "shapes.h"
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
int blurMacGrid(MACGrid& oG, MACGrid& tG, float si);
int blurRealGrid(Grid<Real>& oG, Grid<Real>& tG, float si);
Vec3 calcCenterOfMass(const Grid<Real>& density);
void projectPpmFull(const Grid<Real>& val, std::string name, int shadeMode, Real scale);
void getLaplacian(Grid<Real>& laplacian, const Grid<Real>& grid);
void getCurvature(Grid<Real>& curv, const Grid<Real>& grid, const Real h);
void advectSemiLagrange(const FlagGrid* flags, const MACGrid* vel, GridBase* grid, int order, Real strength, int orderSpace, bool openBounds,
                        int boundaryWidth, int clampMode, int orderTrace);
void setWallBcs(const FlagGrid& flags, MACGrid& vel, const MACGrid* obvel, const MACGrid* fractions, const Grid<Real>* phiObs, int boundaryWidth);
void addBuoyancy(const FlagGrid& flags, const Grid<Real>& density, MACGrid& vel, Vec3 gravity, Real coefficient, bool scale);
void densityInflow(const FlagGrid& flags, Grid<Real>& density, const WaveletNoiseField& noise, Shape* shape, Real scale, Real sigma);
void setOpenBound(FlagGrid& flags, int bWidth, std::string openBound, int type);
void vorticityConfinement(MACGrid& vel, const FlagGrid& flags, Real strength, const Grid<Real>* strengthCell);
void interpolateGrid(Grid<Real>& target, const Grid<Real>& source, Vec3 scale, Vec3 offset, Vec3i size, int orderSpace);
void interpolateMACGrid(MACGrid& target, const MACGrid& source, Vec3 scale, Vec3 offset, Vec3i size, int orderSpace);
void releaseMG(FluidSolver* solver);
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

void load(Grid<Real>& g, const float* a) {
	const IndexInt n = g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ();
	for (IndexInt i = 0; i < n; i++) g[i] = a[i];
}
void store(const Grid<Real>& g, float* a) {
	const IndexInt n = g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ();
	for (IndexInt i = 0; i < n; i++) a[i] = g[i];
}
// Vec3 grids cross element-major: [n][3]
void load3(Grid<Vec3>& g, const float* a) {
	const IndexInt n = g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ();
	for (IndexInt i = 0; i < n; i++) g[i] = Vec3(a[3 * i], a[3 * i + 1], a[3 * i + 2]);
}
void store3(const Grid<Vec3>& g, float* a) {
	const IndexInt n = g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ();
	for (IndexInt i = 0; i < n; i++)
		for (int c = 0; c < 3; c++) a[3 * i + c] = g[i][c];
}

// SoA [3][n]
void storeMac(const Grid<Vec3>& g, float* a) {
	const IndexInt n = g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ();
	for (IndexInt i = 0; i < n; i++)
		for (int c = 0; c < 3; c++) a[c * n + i] = g[i][c];
}

// solvePressure with the reference's own debug line (pressure.cpp:442) captured: the CG iteration count of the solve
struct Solve {
	int iterations;
	template <class F>
	explicit Solve(F call) : iterations(-1) {
		std::ostringstream buf;
		std::streambuf* old = std::cout.rdbuf(buf.rdbuf());
		gDebugLevel = 2;
		try {
			call();
		} catch (...) {
			std::cout.rdbuf(old);
			gDebugLevel = 0;
			throw;
		}
		std::cout.rdbuf(old);
		gDebugLevel = 0;
		const std::string out = buf.str();
		const size_t p = out.rfind("Iterations:");
		if (p != std::string::npos) iterations = atoi(out.c_str() + p + strlen("Iterations:"));
	}
};

// Shape::applyToGrid on a MACGrid is compiled out of the NOPYTHON packaging: its kernel, ApplyShapeToMACGrid (shapes.cpp:62-69)
void applyToMac(MACGrid& grid, const Shape& shape, Vec3 value) {
	FOR_IJK(grid) {
		if (shape.isInside(Vec3(i, j + 0.5, k + 0.5))) grid(i, j, k).x = value.x;
		if (shape.isInside(Vec3(i + 0.5, j, k + 0.5))) grid(i, j, k).y = value.y;
		if (shape.isInside(Vec3(i + 0.5, j + 0.5, k))) grid(i, j, k).z = value.z;
	}
}

void noiseParams(WaveletNoiseField& n, float posScale, float valOffset, float timeAnim) {
	n.mPosScale = Vec3(posScale);
	n.mClamp = true;
	n.mClampNeg = 0;
	n.mClampPos = 1.0;
	n.mValScale = 1.0;
	n.mValOffset = valOffset;
	n.mTimeAnim = timeAnim;
	n.mPosOffset = Vec3(1.5);
}

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* ncomp 1: blurRealGrid on float [n]; ncomp 3: blurMacGrid on float [n][3].  inplace != 0: oG is tG (src is ignored, dst is both).
 * src_after (nullable): oG after the call. */
int rec_blur(int sx, int sy, int sz, int ncomp, const float* src, float* dst, float sigma, int inplace, int* mdim, float* src_after) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	if (ncomp == 1) {
		Grid<Real> o(&s), t(&s);
		load(o, src);
		load(t, dst);
		if (inplace) { load(t, src); *mdim = blurRealGrid(t, t, sigma); }
		else *mdim = blurRealGrid(o, t, sigma);
		store(t, dst);
		if (src_after) store(o, src_after);
	} else {
		MACGrid o(&s), t(&s);
		load3(o, src);
		load3(t, dst);
		if (inplace) { load3(t, src); *mdim = blurMacGrid(t, t, sigma); }
		else *mdim = blurMacGrid(o, t, sigma);
		store3(t, dst);
		if (src_after) store3(o, src_after);
	}
	REC_CATCH
}

int rec_center_of_mass(int sx, int sy, int sz, const float* density, float* out3) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> d(&s);
	load(d, density);
	const Vec3 c = calcCenterOfMass(d);
	for (int q = 0; q < 3; q++) out3[q] = c[q];
	REC_CATCH
}

int rec_project(int sx, int sy, int sz, const float* val, const char* name, int shadeMode, float scale) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> v(&s);
	load(v, val);
	projectPpmFull(v, name, shadeMode, scale);
	REC_CATCH
}

/* out holds the caller's sentinel on entry: the border keeps it */
int rec_laplacian(int sx, int sy, int sz, const float* grid, float* out) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> g(&s), l(&s);
	load(g, grid);
	load(l, out);
	getLaplacian(l, g);
	store(l, out);
	REC_CATCH
}

int rec_curvature(int sx, int sy, int sz, const float* grid, float* out, float h) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> g(&s), c(&s);
	load(g, grid);
	load(c, out);
	getCurvature(c, g, h);
	store(c, out);
	REC_CATCH
}

/* scenes/surfaceTension.py's main loop at res^3 (3-D) for `steps` steps, without the mesh line.  iterations [steps]; phi, curv [n];
 * vel SoA [3][n]. */
int rec_surface_tension(int res, int steps, int* iterations, float* phiOut, float* velOut, float* curvOut) {
	REC_TRY
	gDebugLevel = 0;
	const Vec3 gs(res, res, res);
	FluidSolver s(Vec3i(res, res, res), 3);
	s.mDt = 0.25;
	Grid<Real> curv(&s), pressure(&s);
	FlagGrid flags(&s);
	MACGrid vel(&s);
	LevelsetGrid phi(&s);
	flags.initDomain(1, "xXyYzZ", "      ", "      ", "      ", nullptr);
	Box fluidbox(&s, Vec3::Invalid, gs * Vec3(0.25, 0.25, 0.25), gs * Vec3(0.75, 0.75, 0.75));
	{
		LevelsetGrid a = fluidbox.computeLevelset();
		phi.copyFrom(a);
	}
	flags.updateFromLevelset(phi);
	for (int t = 0; t < steps; t++) {
		phi.reinitMarching(flags, 4.0, &vel, false, true, FlagGrid::TypeObstacle);
		advectSemiLagrange(&flags, &vel, &phi, 1, 1.0, 1, false, -1, 2, 1);
		phi.setBoundNeumann(1);
		flags.updateFromLevelset(phi);
		advectSemiLagrange(&flags, &vel, &vel, 2, 1.0, 1, false, -1, 2, 1);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		getCurvature(curv, phi, 1.0);
		iterations[t] = Solve([&] {
			solvePressure(vel, pressure, flags, 5e-4, &phi, nullptr, nullptr, nullptr, 1e-4, 1.5, true, 1, false, false, false, &curv, 0.1, nullptr);
		}).iterations;
		s.step();
	}
	store(phi, phiOut);
	store(curv, curvOut);
	storeMac(vel, velOut);
	REC_CATCH
}

/* The simMode == 1 loop of tensorflow/example3_resnet/manta_genSimData2.py in 3-D with re-centring on, the script's random draws
 * replaced by the constants of tests/datagen_model.py (LOOP): coarse grid res^3, fine grid (2 res)^3, two density sources (the second
 * an inflow), two initial-velocity spheres, PcMGStatic, resetN = 2, vorticity confinement while t < warm.  src [2][9]: fine centre,
 * coarse centre, scale of the density spheres; srcr [2][2]: fine and coarse radius; seeds [2]; noise [2][3]: posScale, valOffset, fine
 * timeAnim; ini [2][14]: fine centre, fine radius, fine velocity, coarse centre, coarse radius, coarse velocity; buoy [2]: the y
 * gravity of the fine and of the coarse solver.  iterations [steps][2]: fine and coarse solve (-1: no solve in that step); com
 * [steps][3]: calcCenterOfMass of the fine density at the start of each step.  Outputs: coarse density [n], coarse vel SoA [3][n],
 * fine density [N]; the two .ppm files of projectPpmFull(.., 0, 5.0). */
int rec_datagen_loop(int res, int steps, int warm, const float* src, const float* srcr, const int* seeds, const float* noisePar, const float* ini,
                     const float* buoy, int* iterations, float* com, float* densOut, float* velOut, float* xlDensOut, const char* ppmHigh,
                     const char* ppmLow) {
	REC_TRY
	gDebugLevel = 0;
	const int scaleFactor = 2, resetN = 2, bWidth = 1;
	const Vec3i smi(res, res, res), xli(2 * res, 2 * res, 2 * res);
	const Vec3 xl_gs(xli.x, xli.y, xli.z);
	FluidSolver sm(smi, 3), xl(xli, 3);
	FlagGrid flags(&sm), xl_flags(&xl);
	MACGrid vel(&sm), velRecenter(&sm), xl_vel(&xl), xl_velTmp(&xl), xl_velRecenter(&xl);
	Grid<Real> density(&sm), tmp(&sm), xl_density(&xl), xl_tmp(&xl);
	flags.initDomain(bWidth, "xXyYzZ", "      ", "      ", "      ", nullptr);
	flags.fillGrid();
	xl_flags.initDomain(bWidth, "xXyYzZ", "      ", "      ", "      ", nullptr);
	xl_flags.fillGrid();
	setOpenBound(flags, bWidth, "yY", FlagGrid::TypeOutflow | FlagGrid::TypeEmpty);
	setOpenBound(xl_flags, bWidth, "yY", FlagGrid::TypeOutflow | FlagGrid::TypeEmpty);
	WaveletNoiseField* noise[2];
	WaveletNoiseField* noiSm[2];
	Sphere* sources[2];
	Sphere* sourSm[2];
	for (int q = 0; q < 2; q++) {
		const float* c = src + 9 * q;
		noise[q] = new WaveletNoiseField(&xl, seeds[q], 0);
		noiseParams(*noise[q], noisePar[3 * q], noisePar[3 * q + 1], noisePar[3 * q + 2]);
		noiSm[q] = new WaveletNoiseField(&sm, seeds[q], 0);
		noiseParams(*noiSm[q], noisePar[3 * q], noisePar[3 * q + 1], noisePar[3 * q + 2] / float(scaleFactor));
		sources[q] = new Sphere(&xl, Vec3(c[0], c[1], c[2]), srcr[2 * q], Vec3(c[6], c[7], c[8]));
		sourSm[q] = new Sphere(&sm, Vec3(c[3], c[4], c[5]), srcr[2 * q + 1], Vec3(c[6], c[7], c[8]));
		densityInflow(xl_flags, xl_density, *noise[q], sources[q], 1.0, 1.0);
		densityInflow(flags, density, *noiSm[q], sourSm[q], 1.0, 1.0);
	}
	Sphere* iniXl[2];
	Sphere* iniSm[2];
	Vec3 iniV[2], iniVsm[2];
	for (int q = 0; q < 2; q++) {
		const float* c = ini + 14 * q;
		iniXl[q] = new Sphere(&xl, Vec3(c[0], c[1], c[2]), c[3], Vec3(1, 1, 1));
		iniV[q] = Vec3(c[4], c[5], c[6]);
		iniSm[q] = new Sphere(&sm, Vec3(c[7], c[8], c[9]), c[10], Vec3(1, 1, 1));
		iniVsm[q] = Vec3(c[11], c[12], c[13]);
	}
	const float blurSig = float(scaleFactor) / 3.544908;
	const Vec3 one(1.), zero(0.);
	const Vec3i nosize(-1, -1, -1);
	xl_velTmp.copyFrom(xl_vel);
	blurMacGrid(xl_vel, xl_velTmp, blurSig);
	interpolateMACGrid(vel, xl_velTmp, one, zero, nosize, 1);
	vel.multConst(Vec3(1. / scaleFactor));
	for (int t = 0; t < steps; t++) {
		const Vec3 newCentre = calcCenterOfMass(xl_density);
		for (int q = 0; q < 3; q++) com[3 * t + q] = newCentre[q];
		Vec3 xl_velOffset = xl_gs * float(0.5) - newCentre;
		xl_velOffset = xl_velOffset * (1. / xl.getDt());
		const Vec3 velOffset = xl_velOffset * (1. / float(scaleFactor));
		densityInflow(xl_flags, xl_density, *noise[1], sources[1], 1.0, 1.0);
		densityInflow(flags, density, *noiSm[1], sourSm[1], 1.0, 1.0);
		// high res fluid
		advectSemiLagrange(&xl_flags, &xl_velRecenter, &xl_vel, 2, 1.0, 1, true, bWidth, 2, 1);
		setWallBcs(xl_flags, xl_vel, nullptr, nullptr, nullptr, 0);
		addBuoyancy(xl_flags, xl_density, xl_vel, Vec3(0, buoy[0], 0), 1., true);
		for (int q = 0; q < 2; q++) applyToMac(xl_vel, *iniXl[q], iniV[q]);
		if (t < warm) vorticityConfinement(xl_vel, xl_flags, 0.05, nullptr);
		iterations[2 * t] = Solve([&] {
			solvePressure(xl_vel, xl_tmp, xl_flags, 0.001, nullptr, nullptr, nullptr, nullptr, 1e-4, 2.0, true, 3, false, false, false, nullptr, 0., nullptr);
		}).iterations;
		iterations[2 * t + 1] = -1;
		setWallBcs(xl_flags, xl_vel, nullptr, nullptr, nullptr, 0);
		xl_velRecenter.copyFrom(xl_vel);
		xl_velRecenter.addConst(xl_velOffset);
		advectSemiLagrange(&xl_flags, &xl_velRecenter, &xl_density, 2, 1.0, 1, true, bWidth, 2, 1);
		// low res fluid, velocity
		if (t % resetN == 0) {
			xl_velTmp.copyFrom(xl_vel);
			blurMacGrid(xl_vel, xl_velTmp, blurSig);
			interpolateMACGrid(vel, xl_velTmp, one, zero, nosize, 1);
			vel.multConst(Vec3(1. / scaleFactor));
		} else {
			advectSemiLagrange(&flags, &velRecenter, &vel, 2, 1.0, 1, true, bWidth, 2, 1);
			setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
			addBuoyancy(flags, density, vel, Vec3(0, buoy[1], 0), 1., true);
			for (int q = 0; q < 2; q++) applyToMac(vel, *iniSm[q], iniVsm[q]);
			if (t < warm) vorticityConfinement(vel, flags, 0.05 / scaleFactor, nullptr);
			iterations[2 * t + 1] = Solve([&] {
				solvePressure(vel, tmp, flags, 0.001, nullptr, nullptr, nullptr, nullptr, 1e-4, 2.0, true, 3, false, false, false, nullptr, 0., nullptr);
			}).iterations;
			setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		}
		velRecenter.copyFrom(vel);
		velRecenter.addConst(velOffset);
		// low res fluid, density
		if (t % resetN == 0) {
			xl_tmp.copyFrom(xl_density);
			blurRealGrid(xl_density, xl_tmp, blurSig);
			interpolateGrid(density, xl_tmp, one, zero, nosize, 1);
		} else {
			advectSemiLagrange(&flags, &velRecenter, &density, 2, 1.0, 1, true, bWidth, 2, 1);
		}
		sm.step();
		xl.step();
	}
	projectPpmFull(xl_density, ppmHigh, 0, 5.0);
	projectPpmFull(density, ppmLow, 0, 5.0);
	store(density, densOut);
	storeMac(vel, velOut);
	store(xl_density, xlDensOut);
	releaseMG(&sm);
	releaseMG(&xl);
	for (int q = 0; q < 2; q++) {
		delete noise[q];
		delete noiSm[q];
		delete sources[q];
		delete sourSm[q];
		delete iniXl[q];
		delete iniSm[q];
	}
	REC_CATCH
}

}  // extern "C"
