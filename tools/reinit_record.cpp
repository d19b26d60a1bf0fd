/*
 * tools/reinit_record.cpp -- the C++ half of the recorder of tests/golden/reinit.npz (tools/record_reinit.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / grid objects around
 * caller-owned arrays and calls the reference's own LevelsetGrid::reinitMarching (levelset.cpp and fastmarch.cpp are part of
 * oracle/ref.mk's library).  It is compiled in a scratch directory and linked against oracle/_ref/libmanta_ref.so.  No test runs it;
 * nothing it is compiled with is committed.  vel crosses as SoA [3][n].
 */
#include "manta.h"
#include "grid.h"
#include "levelset.h"
#include "shapes.h"
#include <chrono>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void advectSemiLagrange(const FlagGrid* flags, const MACGrid* vel, GridBase* grid, int order, Real strength, int orderSpace, bool openBounds,
                        int boundaryWidth, int clampMode, int orderTrace);
void setWallBcs(const FlagGrid& flags, MACGrid& vel, const MACGrid* obvel, const MACGrid* fractions, const Grid<Real>* phiObs, int boundaryWidth);
void addGravity(const FlagGrid& flags, MACGrid& vel, Vec3 gravity, const Grid<Real>* exclude, bool scale);
void solvePressure(MACGrid& vel, Grid<Real>& pressure, const FlagGrid& flags, Real cgAccuracy, const Grid<Real>* phi,
                   const Grid<Real>* perCellCorr, const MACGrid* fractions, const MACGrid* obvel, Real gfClamp, Real cgMaxIterFac,
                   bool precondition, int preconditioner, bool enforceCompatibility, bool useL2Norm, bool zeroPressureFixing,
                   const Grid<Real>* curv, const Real surfTens, Grid<Real>* retRhs);
extern int gDebugLevel;
}
using namespace Manta;

static std::string g_err;

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* phi.reinitMarching(flags, maxTime, vel (nullable), ignoreWalls, correctOuterLayer, obstacleType) on a solver of (sx, sy, sz), 2-D when
 * sz == 1; *seconds = the wall time of the call alone */
int rec_reinit(int sx, int sy, int sz, float* phi, const int32_t* flags, float* vel, float maxTime, int ignoreWalls, int correctOuterLayer,
               int obstacleType, double* seconds) {
	try {
		gDebugLevel = 0;
		FluidSolver s(Vec3i(sx, sy, sz), sz == 1 ? 2 : 3);
		LevelsetGrid ls(&s);
		FlagGrid fl(&s);
		MACGrid v(&s);
		const IndexInt cells = (IndexInt)sx * sy * sz;
		for (IndexInt i = 0; i < cells; i++) {
			ls[i] = phi[i];
			fl[i] = flags[i];
			if (vel) v[i] = Vec3(vel[i], vel[cells + i], vel[2 * cells + i]);
		}
		const auto t0 = std::chrono::steady_clock::now();
		ls.reinitMarching(fl, maxTime, vel ? &v : nullptr, ignoreWalls != 0, correctOuterLayer != 0, obstacleType);
		*seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		for (IndexInt i = 0; i < cells; i++) {
			phi[i] = ls[i];
			if (vel) {
				vel[i] = v[i].x;
				vel[cells + i] = v[i].y;
				vel[2 * cells + i] = v[i].z;
			}
		}
	} catch (std::exception& e) {
		g_err = e.what();
		return 1;
	}
	return 0;
}

/* The loop of tools/tests/test_2050_freesurface.py (scene 0: basin and drop, dt 0.25, gravity -0.025) or of test_2045_fallingDrop.py
 * (scene 1: a box of liquid, dt 0.6, gravity -0.0125) on (sx, sy, sz), 2-D when sz == 1, res = sx, for `steps` steps, cgAccuracy 5e-5.
 * phi0 = the level set the shapes give before the first step.  The CG iteration count of a step is read from the reference's own debug
 * line (pressure.cpp:442).  phiIn / flagsIn / velIn [steps][n] ([steps][3][n]) = what each step's reinitMarching is given. */
int rec_liquid_loop(int sx, int sy, int sz, int steps, int scene, int* iterations, float* phi0, float* phiOut, float* velOut, float* phiIn,
                    int32_t* flagsIn, float* velIn) {
	try {
		gDebugLevel = 0;
		const int res = sx;
		const Vec3 gs(sx, sy, sz);
		FluidSolver s(Vec3i(sx, sy, sz), sz == 1 ? 2 : 3);
		s.mDt = scene == 0 ? 0.25 : 0.6;
		FlagGrid flags(&s);
		MACGrid vel(&s);
		Grid<Real> pressure(&s);
		LevelsetGrid phi(&s);
		flags.initDomain(0, "xXyYzZ", "      ", "      ", "      ", nullptr);
		if (scene == 0) {
			Box basin(&s, Vec3::Invalid, gs * Vec3(0, 0, 0), gs * Vec3(1, 0.2, 1));
			Sphere drop(&s, gs * Vec3(0.5, 0.5, 0.5), res * 0.15);
			LevelsetGrid a = basin.computeLevelset(), b = drop.computeLevelset();
			phi.copyFrom(a);
			phi.join(b);
		} else {
			Box liq(&s, Vec3::Invalid, gs * Vec3(0.4, 0.75, 0.4), gs * Vec3(0.6, 0.95, 0.6));
			LevelsetGrid a = liq.computeLevelset();
			phi.copyFrom(a);
		}
		flags.updateFromLevelset(phi);
		const IndexInt cells = (IndexInt)sx * sy * sz;
		for (IndexInt i = 0; i < cells; i++) phi0[i] = phi[i];
		for (int step = 0; step < steps; step++) {
			for (IndexInt i = 0; i < cells; i++) {
				phiIn[step * cells + i] = phi[i];
				flagsIn[step * cells + i] = flags[i];
				velIn[(3 * step) * cells + i] = vel[i].x;
				velIn[(3 * step + 1) * cells + i] = vel[i].y;
				velIn[(3 * step + 2) * cells + i] = vel[i].z;
			}
			phi.reinitMarching(flags, 4.0, &vel, false, true, FlagGrid::TypeObstacle);
			advectSemiLagrange(&flags, &vel, &phi, 2, 1.0, 1, false, -1, 1, 1);
			flags.updateFromLevelset(phi);
			advectSemiLagrange(&flags, &vel, &vel, 2, 1.0, 1, false, -1, 1, 1);
			addGravity(flags, vel, Vec3(0, scene == 0 ? -0.025 : -0.0125, 0), nullptr, true);
			setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
			{
				std::ostringstream buf;
				std::streambuf* old = std::cout.rdbuf(buf.rdbuf());
				gDebugLevel = 2;
				try {
					solvePressure(vel, pressure, flags, 5e-5, &phi, nullptr, nullptr, nullptr, 1e-4, 0.5, true, 1, false, false, false, nullptr, 0., nullptr);
				} catch (...) {
					std::cout.rdbuf(old);
					gDebugLevel = 0;
					throw;
				}
				std::cout.rdbuf(old);
				gDebugLevel = 0;
				const std::string out = buf.str();
				const size_t p = out.rfind("Iterations:");
				iterations[step] = p == std::string::npos ? -1 : atoi(out.c_str() + p + strlen("Iterations:"));
			}
			setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
			s.step();
		}
		for (IndexInt i = 0; i < cells; i++) {
			phiOut[i] = phi[i];
			velOut[i] = vel[i].x;
			velOut[cells + i] = vel[i].y;
			velOut[2 * cells + i] = vel[i].z;
		}
	} catch (std::exception& e) {
		g_err = e.what();
		return 1;
	}
	return 0;
}

}  // extern "C"
