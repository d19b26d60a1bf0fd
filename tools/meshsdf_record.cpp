/*
 * tools/meshsdf_record.cpp -- the C++ half of the recorder of tests/golden/meshsdf.npz (tools/record_meshsdf.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Mesh / grid objects around
 * caller-owned arrays and calls the reference's own Mesh::computeLevelset and densityInflowMesh (mesh.cpp and plugin/initplugins.cpp
 * are part of oracle/ref.mk's library).  It is compiled in a scratch directory and linked against oracle/_ref/libmanta_ref.so.  No test
 * runs it; nothing it is compiled with is committed.  Meshes cross as [n][3] arrays.
 */
#include "manta.h"
#include "grid.h"
#include "levelset.h"
#include "mesh.h"
#include "shapes.h"
#include <chrono>
#include <iostream>
#include <sstream>
#include <cstring>
#include <string>

namespace Manta {
// PYTHON() plugin (a plain function in the NOPYTHON packaging; no header declares it)
void densityInflowMesh(const FlagGrid& flags, Grid<Real>& density, Mesh* mesh, Real value, Real cutoff, Real sigma);
void advectSemiLagrange(const FlagGrid* flags, const MACGrid* vel, GridBase* grid, int order, Real strength, int orderSpace, bool openBounds,
                        int boundaryWidth, int clampMode, int orderTrace);
void setWallBcs(const FlagGrid& flags, MACGrid& vel, const MACGrid* obvel, const MACGrid* fractions, const Grid<Real>* phiObs, int boundaryWidth);
void addBuoyancy(const FlagGrid& flags, const Grid<Real>& density, MACGrid& vel, Vec3 gravity, Real coefficient, bool scale);
void solvePressure(MACGrid& vel, Grid<Real>& pressure, const FlagGrid& flags, Real cgAccuracy, const Grid<Real>* phi,
                   const Grid<Real>* perCellCorr, const MACGrid* fractions, const MACGrid* obvel, Real gfClamp, Real cgMaxIterFac,
                   bool precondition, int preconditioner, bool enforceCompatibility, bool useL2Norm, bool zeroPressureFixing,
                   const Grid<Real>* curv, const Real surfTens, Grid<Real>* retRhs);
void setObstacleFlags(FlagGrid& flags, const Grid<Real>& phiObs, const MACGrid* fractions, const Grid<Real>* phiOut, const Grid<Real>* phiIn,
                      int boundaryWidth);
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

static void fill(Mesh& m, int64_t n, const float* pos, int64_t t, const int32_t* tris) {
	for (int64_t i = 0; i < n; i++) {
		Node nd;
		nd.pos = Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
		m.addNode(nd);
	}
	for (int64_t i = 0; i < t; i++) m.addTri(Triangle(tris[3 * i], tris[3 * i + 1], tris[3 * i + 2]));
}

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* Mesh::computeLevelset of a mesh that lives in a solver of (gx, gy, gz) on a level set of (sx, sy, sz), which starts as NaN;
 * *seconds = the wall time of the call alone */
int rec_compute_levelset(int gx, int gy, int gz, int64_t n, const float* pos, int64_t t, const int32_t* tris, int sx, int sy, int sz,
                         float sigma, float cutoff, float* phi, double* seconds) {
	REC_TRY
	gDebugLevel = 0;
	FluidSolver ms(Vec3i(gx, gy, gz), 3), gs(Vec3i(sx, sy, sz), 3);
	Mesh m(&ms);
	fill(m, n, pos, t, tris);
	LevelsetGrid ls(&gs);
	const IndexInt cells = (IndexInt)sx * sy * sz;
	for (IndexInt i = 0; i < cells; i++) ls[i] = std::numeric_limits<Real>::quiet_NaN();
	const auto t0 = std::chrono::steady_clock::now();
	m.computeLevelset(ls, sigma, cutoff);
	*seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	for (IndexInt i = 0; i < cells; i++) phi[i] = ls[i];
	REC_CATCH
}

/* densityInflowMesh on caller-owned flags and density */
int rec_density_inflow_mesh(int sx, int sy, int sz, int64_t n, const float* pos, int64_t t, const int32_t* tris, const int32_t* flags,
                            float* density, float value, float cutoff, float sigma) {
	REC_TRY
	gDebugLevel = 0;
	FluidSolver s(Vec3i(sx, sy, sz), 3);
	Mesh m(&s);
	fill(m, n, pos, t, tris);
	FlagGrid fl(&s);
	Grid<Real> dens(&s);
	const IndexInt cells = (IndexInt)sx * sy * sz;
	for (IndexInt i = 0; i < cells; i++) {
		fl[i] = flags[i];
		dens[i] = density[i];
	}
	densityInflowMesh(fl, dens, &m, value, cutoff, sigma);
	for (IndexInt i = 0; i < cells; i++) density[i] = dens[i];
	REC_CATCH
}

/* the loop of scenes/meshload.py at res^3 on a mesh already placed: computeLevelset(phiObs, 2.), initDomain, setObstacleFlags,
 * fillGrid, then `steps` smoke steps.  cyl = centre, radius, z of the script's source cylinder as the caller's floats; its
 * applyToGrid(value = 1) is compiled out under NOPYTHON and written here as its kernel, ApplyShapeToGrid (shapes.cpp:41-47).  The CG
 * iteration count of a step is read from the reference's own debug line (pressure.cpp:442).  vel crosses as SoA [3][n]. */
int rec_meshload_loop(int res, int steps, int64_t n, const float* pos, int64_t t, const int32_t* tris, const float* cyl, int32_t* flagsOut,
                      int* iterations, float* density, float* vel, float* pressure) {
	REC_TRY
	gDebugLevel = 0;
	FluidSolver s(Vec3i(res, res, res), 3);
	FlagGrid flags(&s);
	Grid<Real> dens(&s), pres(&s);
	MACGrid v(&s);
	LevelsetGrid phiObs(&s);
	Mesh m(&s);
	fill(m, n, pos, t, tris);
	m.computeLevelset(phiObs, 2., -1.);
	flags.initDomain(0, "xXyYzZ", "      ", "      ", "      ", nullptr);
	setObstacleFlags(flags, phiObs, nullptr, nullptr, nullptr, 1);
	flags.fillGrid();
	Cylinder source(&s, Vec3(cyl[0], cyl[1], cyl[2]), cyl[3], Vec3(cyl[4], cyl[5], cyl[6]));
	const IndexInt cells = (IndexInt)res * res * res;
	for (int step = 0; step < steps; step++) {
		FOR_IJK(dens) {
			if (source.isInsideGrid(i, j, k)) dens(i, j, k) = 1.;
		}
		advectSemiLagrange(&flags, &v, &dens, 2, 1.0, 1, false, -1, 2, 1);
		advectSemiLagrange(&flags, &v, &v, 2, 1.0, 1, false, -1, 2, 1);
		setWallBcs(flags, v, nullptr, nullptr, nullptr, 0);
		addBuoyancy(flags, dens, v, Vec3(0, -1e-3, 0), 1., true);
		{
			std::ostringstream buf;
			std::streambuf* old = std::cout.rdbuf(buf.rdbuf());
			gDebugLevel = 2;
			try {
				solvePressure(v, pres, flags, 1e-3, nullptr, nullptr, nullptr, nullptr, 1e-4, 1.5, true, 1, false, false, false, nullptr, 0., nullptr);
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
		s.step();
	}
	for (IndexInt i = 0; i < cells; i++) {
		flagsOut[i] = flags[i];
		density[i] = dens[i];
		pressure[i] = pres[i];
		vel[i] = v[i].x;
		vel[cells + i] = v[i].y;
		vel[2 * cells + i] = v[i].z;
	}
	REC_CATCH
}

}  // extern "C"
