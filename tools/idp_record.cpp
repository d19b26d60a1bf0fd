/*
 * tools/idp_record.cpp -- the C++ half of the recorder of tests/golden/idp.npz (tools/record_idp.py is the other half; its header
 * has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid / BasicParticleSystem
 * objects around caller-owned arrays and calls the reference's own implicit-density-projection plugins, plus the main loop of
 * scenes/idp_apic01_simple.py / idp_apic02_3d.py written against the reference's classes (same calls, same arguments, same order).
 * It is compiled in a scratch directory together with the expanded plugin/implicitdensityprojection.cpp (which oracle/ref.mk does
 * not build) and linked against oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled with is committed.
 *
 * Array conventions are those of include/manta_hip.h: MAC grids and particle vectors are SoA ([3][n]).
 */
#include "manta.h"
#include "grid.h"
#include "particle.h"
#include "levelset.h"
#include "shapes.h"
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void copyFlagsToFlags(FlagGrid& source, FlagGrid& target);
void markFluidAndBoundaryCells(const BasicParticleSystem& particles, FlagGrid& flags, MACGrid& deltaX, const Grid<Real>& phiObs,
                               const ParticleDataImpl<int>* ptype, const int exclude);
void mapMassToGrid(FlagGrid& flags, Grid<Real>& density, const BasicParticleSystem& parts, ParticleDataImpl<Real>& source, MACGrid& deltaX,
                   const Grid<Real>& phiObs, Real dt, Real particleMass, bool noDensityClamping);
void computeDeltaX(MACGrid& deltaX, Grid<Real>& Lambda, const FlagGrid& flags);
void mapMACToPartPositions(const FlagGrid& flags, const MACGrid& deltaX, BasicParticleSystem& parts, Real dt, const ParticleDataImpl<int>* ptype,
                           const int exclude, bool mapQuadratic);
void solvePressureSystem(Grid<Real>& rhs, MACGrid& vel, Grid<Real>& pressure, const FlagGrid& flags, Real cgAccuracy, const Grid<Real>* phi,
                         const Grid<Real>* perCellCorr, const MACGrid* fractions, Real gfClamp, Real cgMaxIterFac, bool precondition,
                         int preconditioner, const bool enforceCompatibility, const bool useL2Norm, const bool zeroPressureFixing,
                         const Grid<Real>* curv, const Real surfTens);
void solvePressure(MACGrid& vel, Grid<Real>& pressure, const FlagGrid& flags, Real cgAccuracy, const Grid<Real>* phi,
                   const Grid<Real>* perCellCorr, const MACGrid* fractions, const MACGrid* obvel, Real gfClamp, Real cgMaxIterFac,
                   bool precondition, int preconditioner, bool enforceCompatibility, bool useL2Norm, bool zeroPressureFixing,
                   const Grid<Real>* curv, const Real surfTens, Grid<Real>* retRhs);
void setWallBcs(const FlagGrid& flags, MACGrid& vel, const MACGrid* obvel, const MACGrid* fractions, const Grid<Real>* phiObs, int boundaryWidth);
void addGravityNoScale(const FlagGrid& flags, MACGrid& vel, const Vec3& gravity, const Grid<Real>* exclude);
void extrapolateMACSimple(FlagGrid& flags, MACGrid& vel, int distance, LevelsetGrid* phiObs, bool intoObs);
void extrapolateMACFromWeight(MACGrid& vel, Grid<Vec3>& weight, int distance);
void markFluidCells(const BasicParticleSystem& parts, FlagGrid& flags, const Grid<Real>* phiObs, const ParticleDataImpl<int>* ptype, const int exclude);
void sampleFlagsWithParticles(const FlagGrid& flags, BasicParticleSystem& parts, const int discretization, const Real randomness);
void apicMapPartsToMAC(const FlagGrid& flags, MACGrid& vel, const BasicParticleSystem& parts, const ParticleDataImpl<Vec3>& partVel,
                       const ParticleDataImpl<Vec3>& cpx, const ParticleDataImpl<Vec3>& cpy, const ParticleDataImpl<Vec3>& cpz, MACGrid* mass,
                       const ParticleDataImpl<int>* ptype, const int exclude);
void apicMapMACGridToParts(ParticleDataImpl<Vec3>& partVel, ParticleDataImpl<Vec3>& cpx, ParticleDataImpl<Vec3>& cpy, ParticleDataImpl<Vec3>& cpz,
                           const BasicParticleSystem& parts, const MACGrid& vel, const FlagGrid& flags, const ParticleDataImpl<int>* ptype,
                           const int exclude);
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
void loadParts(BasicParticleSystem& sys, int64_t np, const float* pos, const int32_t* pflag) {
	sys.resizeAll(np);
	for (int64_t i = 0; i < np; i++) {
		sys[i].pos = Vec3(pos[i], pos[np + i], pos[2 * np + i]);
		sys[i].flag = pflag[i];
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
}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

int rec_mark(int sx, int sy, int sz, int32_t* flags, float* deltaX, const float* phiObs, int64_t np, const float* pos, const int32_t* pflag,
             const int32_t* ptype, int exclude) {
	REC_TRY
	FluidSolver solver(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	const int64_t n = (int64_t)sx * sy * sz;
	FlagGrid fl(&solver, flags);
	Grid<Real> phi(&solver, const_cast<float*>(phiObs));
	MACGrid dX(&solver);
	BasicParticleSystem sys(&solver);
	loadParts(sys, np, pos, pflag);
	ParticleDataImpl<int> pt(&solver);
	sys.registerPdata(&pt);
	pt.resize(np);
	if (ptype)
		for (int64_t i = 0; i < np; i++) pt[i] = ptype[i];
	markFluidAndBoundaryCells(sys, fl, dX, phi, ptype ? &pt : nullptr, exclude);
	storeMac(dX, deltaX, n);
	REC_CATCH
}

int rec_map_mass(int sx, int sy, int sz, int32_t* flags, float* density, float* deltaX, const float* phiObs, int64_t np, const float* pos,
                 const int32_t* pflag, float dt, float mass, int noClamp) {
	REC_TRY
	FluidSolver solver(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	const int64_t n = (int64_t)sx * sy * sz;
	FlagGrid fl(&solver, flags);
	Grid<Real> phi(&solver, const_cast<float*>(phiObs)), dens(&solver, density);
	MACGrid dX(&solver);
	BasicParticleSystem sys(&solver);
	loadParts(sys, np, pos, pflag);
	ParticleDataImpl<Real> src(&solver);
	sys.registerPdata(&src);
	src.resize(np);
	mapMassToGrid(fl, dens, sys, src, dX, phi, dt, mass, noClamp != 0);
	storeMac(dX, deltaX, n);
	REC_CATCH
}

int rec_compute_delta_x(int sx, int sy, int sz, float* deltaX, float* Lambda, const int32_t* flags) {
	REC_TRY
	FluidSolver solver(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	const int64_t n = (int64_t)sx * sy * sz;
	FlagGrid fl(&solver, const_cast<int32_t*>(flags));
	Grid<Real> L(&solver, Lambda);
	MACGrid dX(&solver);
	loadMac(dX, deltaX, n);
	computeDeltaX(dX, L, fl);
	storeMac(dX, deltaX, n);
	REC_CATCH
}

int rec_map_positions(int sx, int sy, int sz, const float* deltaX, int64_t np, float* pos, const int32_t* pflag, float dt, const int32_t* ptype,
                      int exclude) {
	REC_TRY
	FluidSolver solver(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	const int64_t n = (int64_t)sx * sy * sz;
	FlagGrid fl(&solver);
	MACGrid dX(&solver);
	loadMac(dX, deltaX, n);
	BasicParticleSystem sys(&solver);
	loadParts(sys, np, pos, pflag);
	ParticleDataImpl<int> pt(&solver);
	sys.registerPdata(&pt);
	pt.resize(np);
	if (ptype)
		for (int64_t i = 0; i < np; i++) pt[i] = ptype[i];
	mapMACToPartPositions(fl, dX, sys, dt, ptype ? &pt : nullptr, exclude, false);
	for (int64_t i = 0; i < np; i++) {
		pos[i] = sys[i].pos.x;
		pos[np + i] = sys[i].pos.y;
		pos[2 * np + i] = sys[i].pos.z;
	}
	REC_CATCH
}

/* the scenes' main loop.  per_step: [steps][3] = dt, CG iterations of the position solve, of the pressure solve; grids: density,
 * Lambda [n], deltaX, vel [3][n], flags, flagsPos [n]; pos: [3][pos_cap] (np_out particles). */
int rec_loop(int res, int dim, int steps, float cfl, float* per_step, float* density_out, float* lambda_out, float* deltaX_out, float* vel_out,
             int32_t* flags_out, int32_t* flagsPos_out, int64_t pos_cap, float* pos_out, int64_t* np_out) {
	REC_TRY
	const int particleNumber = dim == 3 ? 2 : 3;
	const Vec3i gsi(res, res, dim == 3 ? res : 1);
	const Vec3 gs(gsi.x, gsi.y, gsi.z);
	FluidSolver s(gsi, dim);
	FlagGrid flags(&s), flagsPos(&s);
	MACGrid vel(&s), apic_mass(&s), deltaX(&s);
	Grid<Real> pressure(&s), density(&s), Lambda(&s);
	Grid<Vec3> tmpVec3(&s);
	LevelsetGrid phiObs(&s);
	BasicParticleSystem pp(&s);
	ParticleDataImpl<Vec3> pVel(&s), cpx(&s), cpy(&s), cpz(&s);
	ParticleDataImpl<Real> pMass(&s);
	pp.registerPdata(&pVel);
	pp.registerPdata(&cpx);
	pp.registerPdata(&cpy);
	pp.registerPdata(&cpz);
	pp.registerPdata(&pMass);
	const Real mass = dim == 3 ? 1.0 / (particleNumber * particleNumber * particleNumber) : 1.0 / (particleNumber * particleNumber);
	s.mDt = 1;
	s.mFrameLength = 10000000.0;
	s.mDtMin = 0.01;
	s.mDtMax = 1.0;
	s.mCflCond = cfl;
	flags.initDomain(1, "xXyYzZ", "      ", "      ", "      ", nullptr);
	Box box(&s, Vec3::Invalid, dim == 3 ? gs * Vec3(0, 0, 0.25) : gs * Vec3(0, 0, 0), dim == 3 ? gs * Vec3(0.5, 0.35, 0.75) : gs * Vec3(0.4, 0.6, 1),
	        Vec3::Invalid);
	LevelsetGrid phiInit = box.computeLevelset();
	flags.updateFromLevelset(phiInit);
	sampleFlagsWithParticles(flags, pp, particleNumber, 0.5);
	copyFlagsToFlags(flags, flagsPos);
	flags.initDomain(1, "xXyYzZ", "      ", "      ", "      ", &phiObs);
	const Vec3 gravity(0, dim == 3 ? -0.01 : -0.002, 0);
	for (int t = 0; t < steps; t++) {
		s.adaptTimestep(vel.getMax());
		per_step[3 * t] = s.mDt;
		pp.advectInGrid(flags, vel, 2, false, false, false, nullptr, 0);
		copyFlagsToFlags(flags, flagsPos);
		mapMassToGrid(flagsPos, density, pp, pMass, deltaX, phiObs, s.mDt, mass, false);
		{   // what the step exercises (for choosing resolution and step count): particles inside obstacle cells, cells with particles left empty
			int inObs = 0;
			Grid<int> seen(&s);
			for (IndexInt i = 0; i < pp.size(); i++) {
				const Vec3i c = toVec3i(pp[i].pos);
				if (!pp.isActive(i) || !flags.isInBounds(c)) continue;
				if (flagsPos.isObstacle(c)) inObs++;
				else seen(c) = 1;
			}
			int flipped = 0;
			FOR_IDX(seen) if (seen[idx] && flagsPos[idx] == FlagGrid::TypeEmpty) flipped++;
			std::cerr << "step " << t << ": " << inObs << " particles in obstacle cells, " << flipped << " cells flipped" << std::endl;
		}
		{
			Capture c;
			solvePressureSystem(density, vel, Lambda, flagsPos, 1e-3, nullptr, nullptr, nullptr, 1e-04, 1.5, true, 1, false, false, false, nullptr, 0.);
			per_step[3 * t + 1] = c.iterations();
		}
		computeDeltaX(deltaX, Lambda, flagsPos);
		mapMACToPartPositions(flagsPos, deltaX, pp, s.mDt, nullptr, 0, false);
		apicMapPartsToMAC(flags, vel, pp, pVel, cpx, cpy, cpz, &apic_mass, nullptr, 0);
		extrapolateMACFromWeight(vel, tmpVec3, 2);
		markFluidCells(pp, flags, nullptr, nullptr, 0);
		addGravityNoScale(flags, vel, gravity, nullptr);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		{
			Capture c;
			solvePressure(vel, pressure, flags, 1e-3, nullptr, nullptr, nullptr, nullptr, 1e-04, 1.5, true, 1, false, false, false, nullptr, 0., nullptr);
			per_step[3 * t + 2] = c.iterations();
		}
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		extrapolateMACSimple(flags, vel, 5, nullptr, false);
		apicMapMACGridToParts(pVel, cpx, cpy, cpz, pp, vel, flags, nullptr, 0);
		s.step();
	}
	const int64_t n = (int64_t)gsi.x * gsi.y * gsi.z;
	for (int64_t i = 0; i < n; i++) {
		density_out[i] = density[i];
		lambda_out[i] = Lambda[i];
		flags_out[i] = flags[i];
		flagsPos_out[i] = flagsPos[i];
	}
	storeMac(deltaX, deltaX_out, n);
	storeMac(vel, vel_out, n);
	const int64_t np = pp.size();
	if (np > pos_cap) throw std::runtime_error("rec_loop: pos_cap too small");
	*np_out = np;
	for (int64_t i = 0; i < np; i++) {
		pos_out[i] = pp[i].pos.x;
		pos_out[pos_cap + i] = pp[i].pos.y;
		pos_out[2 * pos_cap + i] = pp[i].pos.z;
	}
	REC_CATCH
}

}  // extern "C"
