/*
 * tools/partls_record.cpp -- the C++ half of the recorder of tests/golden/partls.npz (tools/record_partls.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid / BasicParticleSystem
 * objects around caller-owned arrays and calls the reference's own gridParticleIndex, averagedParticleLevelset and
 * improvedParticleLevelset (plugin/flip.cpp is part of oracle/ref.mk's library, so they are only declared here), plus the step of
 * scenes/flip02_surface.py (dam break, no adjustNumber, no mesh) written against the reference's classes with one of the two level
 * sets in the place of unionParticleLevelset.  It is compiled in a scratch directory and linked against oracle/_ref/libmanta_ref.so.
 * No test runs it; nothing it is compiled with is committed.
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
#include <zlib.h>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void gridParticleIndex(const BasicParticleSystem& parts, ParticleIndexSystem& indexSys, const FlagGrid& flags, Grid<int>& index, Grid<int>* counter);
void averagedParticleLevelset(const BasicParticleSystem& parts, const ParticleIndexSystem& indexSys, const FlagGrid& flags, const Grid<int>& index,
                              LevelsetGrid& phi, const Real radiusFactor, const int smoothen, const int smoothenNeg,
                              const ParticleDataImpl<int>* ptype, const int exclude);
void improvedParticleLevelset(const BasicParticleSystem& parts, const ParticleIndexSystem& indexSys, const FlagGrid& flags, const Grid<int>& index,
                              LevelsetGrid& phi, const Real radiusFactor, const int smoothen, const int smoothenNeg, const Real t_low,
                              const Real t_high, const ParticleDataImpl<int>* ptype, const int exclude);
void sampleLevelsetWithParticles(const LevelsetGrid& phi, const FlagGrid& flags, BasicParticleSystem& parts, const int discretization,
                                 const Real randomness, const bool reset, const bool refillEmpty, const int particleFlag);
void mapPartsToMAC(const FlagGrid& flags, MACGrid& vel, MACGrid& velOld, const BasicParticleSystem& parts, const ParticleDataImpl<Vec3>& partVel,
                   Grid<Vec3>* weight, const ParticleDataImpl<int>* ptype, const int exclude);
void extrapolateMACFromWeight(MACGrid& vel, Grid<Vec3>& weight, int distance);
void markFluidCells(const BasicParticleSystem& parts, FlagGrid& flags, const Grid<Real>* phiObs, const ParticleDataImpl<int>* ptype, const int exclude);
void resetOutflow(FlagGrid& flags, Grid<Real>* phi, BasicParticleSystem* parts, Grid<Real>* real, Grid<int>* index, ParticleIndexSystem* indexSys);
void extrapolateLsSimple(Grid<Real>& phi, int distance, bool inside, bool include_walls);
void addGravity(const FlagGrid& flags, MACGrid& vel, Vec3 gravity, const Grid<Real>* exclude, bool scale);
void setWallBcs(const FlagGrid& flags, MACGrid& vel, const MACGrid* obvel, const MACGrid* fractions, const Grid<Real>* phiObs, int boundaryWidth);
void solvePressure(MACGrid& vel, Grid<Real>& pressure, const FlagGrid& flags, Real cgAccuracy, const Grid<Real>* phi,
                   const Grid<Real>* perCellCorr, const MACGrid* fractions, const MACGrid* obvel, Real gfClamp, Real cgMaxIterFac,
                   bool precondition, int preconditioner, bool enforceCompatibility, bool useL2Norm, bool zeroPressureFixing,
                   const Grid<Real>* curv, const Real surfTens, Grid<Real>* retRhs);
void extrapolateMACSimple(FlagGrid& flags, MACGrid& vel, int distance, LevelsetGrid* phiObs, bool intoObs);
void flipVelocityUpdate(const FlagGrid& flags, const MACGrid& vel, const MACGrid& velOld, const BasicParticleSystem& parts,
                        ParticleDataImpl<Vec3>& partVel, const Real flipRatio, const ParticleDataImpl<int>* ptype, const int exclude);
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

/* one plugin call: pos [3][np] SoA, phi [n] out (pre-filled by the caller), n_indexed out */
int rec_levelset(int sx, int sy, int sz, int64_t np, const float* pos, const int32_t* pflag, const int32_t* ptype, int exclude, int improved,
                 float radiusFactor, int smoothen, int smoothenNeg, float t_low, float t_high, float* phi_out, int64_t* n_indexed) {
	REC_TRY
	FluidSolver solver(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid flags(&solver);
	Grid<int> index(&solver);
	LevelsetGrid phi(&solver);   // the plugins swap it with their temporary: no external storage
	const int64_t n = (int64_t)sx * sy * sz;
	for (int64_t i = 0; i < n; i++) phi[i] = phi_out[i];
	BasicParticleSystem sys(&solver);
	ParticleIndexSystem isys(&solver);
	sys.resizeAll(np);
	for (int64_t i = 0; i < np; i++) {
		sys[i].pos = Vec3(pos[i], pos[np + i], pos[2 * np + i]);
		sys[i].flag = pflag[i];
	}
	ParticleDataImpl<int> pt(&solver);
	sys.registerPdata(&pt);
	pt.resize(np);
	if (ptype)
		for (int64_t i = 0; i < np; i++) pt[i] = ptype[i];
	gridParticleIndex(sys, isys, flags, index, nullptr);
	*n_indexed = isys.size();
	if (improved) improvedParticleLevelset(sys, isys, flags, index, phi, radiusFactor, smoothen, smoothenNeg, t_low, t_high, ptype ? &pt : nullptr, exclude);
	else averagedParticleLevelset(sys, isys, flags, index, phi, radiusFactor, smoothen, smoothenNeg, ptype ? &pt : nullptr, exclude);
	for (int64_t i = 0; i < n; i++) phi_out[i] = phi[i];
	REC_CATCH
}

/* the FLIP loop.  iters [steps]: CG iterations; crc [steps]: crc32 of phi right after the level-set plugin; phi [n], vel [3][n] and
 * pos [3][pos_cap] (np_out particles) at the end */
int rec_loop(int improved, int res, int steps, int64_t* iters, uint32_t* crc, float* phi_out, float* vel_out, int64_t pos_cap, float* pos_out,
             int64_t* np_out) {
	REC_TRY
	const Vec3i gsi(res, res, res);
	const Vec3 gs(res, res, res);
	FluidSolver s(gsi, 3);
	s.mDt = 0.8;
	FlagGrid flags(&s);
	LevelsetGrid phi(&s);
	MACGrid vel(&s), velOld(&s);
	Grid<Real> pressure(&s);
	Grid<Vec3> tmpVec3(&s);
	BasicParticleSystem pp(&s);
	ParticleDataImpl<Vec3> pVel(&s);
	pp.registerPdata(&pVel);
	ParticleIndexSystem pindex(&s);
	Grid<int> gpi(&s);
	flags.initDomain(1, "xXyYzZ", "      ", "      ", "      ", nullptr);
	Box fluidbox(&s, Vec3::Invalid, gs * Vec3(0, 0, 0), gs * Vec3(0.4, 0.6, 1), Vec3::Invalid);
	LevelsetGrid phiInit = fluidbox.computeLevelset();
	flags.updateFromLevelset(phiInit);
	sampleLevelsetWithParticles(phiInit, flags, pp, 2, 0.05, false, false, -1);
	const int64_t n = (int64_t)res * res * res;
	for (int t = 0; t < steps; t++) {
		pp.advectInGrid(flags, vel, 2 /* IntRK4 */, false, true, false, nullptr, 0);
		mapPartsToMAC(flags, vel, velOld, pp, pVel, &tmpVec3, nullptr, 0);
		extrapolateMACFromWeight(vel, tmpVec3, 2);
		markFluidCells(pp, flags, nullptr, nullptr, 0);
		gridParticleIndex(pp, pindex, flags, gpi, nullptr);
		if (improved) improvedParticleLevelset(pp, pindex, flags, gpi, phi, 1.0, 1, 1, 0.4, 3.5, nullptr, 0);
		else averagedParticleLevelset(pp, pindex, flags, gpi, phi, 1.0, 1, 1, nullptr, 0);
		crc[t] = (uint32_t)crc32(0L, (const Bytef*)&phi[0], (uInt)(n * sizeof(float)));
		resetOutflow(flags, nullptr, &pp, nullptr, &gpi, &pindex);
		extrapolateLsSimple(phi, 4, true, false);
		addGravity(flags, vel, Vec3(0, -0.001, 0), nullptr, true);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		{
			Capture c;
			solvePressure(vel, pressure, flags, 1e-3, &phi, nullptr, nullptr, nullptr, 1e-04, 1.5, true, 1, false, false, false, nullptr, 0., nullptr);
			iters[t] = c.iterations();
		}
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		extrapolateMACSimple(flags, vel, 4, nullptr, false);
		flipVelocityUpdate(flags, vel, velOld, pp, pVel, 0.97, nullptr, 0);
		s.step();
	}
	for (int64_t i = 0; i < n; i++) {
		phi_out[i] = phi[i];
		vel_out[i] = vel[i].x;
		vel_out[n + i] = vel[i].y;
		vel_out[2 * n + i] = vel[i].z;
	}
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
