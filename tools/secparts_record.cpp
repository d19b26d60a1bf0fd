/*
 * tools/secparts_record.cpp -- the C++ half of the recorder of tests/golden/secparts.npz (tools/record_secparts.py is the other half;
 * its header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid /
 * BasicParticleSystem objects around caller-owned arrays and calls the reference's own secondary-particle plugins
 * (plugin/secondaryparticles.cpp is not part of oracle/ref.mk's library: the recorder's commands expand it with the reference's
 * `prep` in a scratch directory and compile it next to this file), plus the step of scenes/flip01_simple.py (3-D dam break) written
 * against the reference's classes with a secondary particle system beside it.  It is compiled in a scratch directory and linked
 * against oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled with is committed.
 */
#include "manta.h"
#include "grid.h"
#include "particle.h"
#include "levelset.h"
#include "shapes.h"
#include <cstring>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void flipComputeSecondaryParticlePotentials(Grid<Real>& potTA, Grid<Real>& potWC, Grid<Real>& potKE, Grid<Real>& neighborRatio, const FlagGrid& flags,
                                            const MACGrid& v, Grid<Vec3>& normal, const Grid<Real>& phi, const int radius, const Real tauMinTA,
                                            const Real tauMaxTA, const Real tauMinWC, const Real tauMaxWC, const Real tauMinKE, const Real tauMaxKE,
                                            const Real scaleFromManta, const int itype, const int jtype);
void flipSampleSecondaryParticles(const std::string mode, const FlagGrid& flags, const MACGrid& v, BasicParticleSystem& pts_sec,
                                  ParticleDataImpl<Vec3>& v_sec, ParticleDataImpl<Real>& l_sec, const Real lMin, const Real lMax,
                                  const Grid<Real>& potTA, const Grid<Real>& potWC, const Grid<Real>& potKE, const Grid<Real>& neighborRatio,
                                  const Real c_s, const Real c_b, const Real k_ta, const Real k_wc, const Real dt, const int itype);
void flipUpdateSecondaryParticles(const std::string mode, BasicParticleSystem& pts_sec, ParticleDataImpl<Vec3>& v_sec, ParticleDataImpl<Real>& l_sec,
                                  const ParticleDataImpl<Vec3>& f_sec, FlagGrid& flags, const MACGrid& v, const Grid<Real>& neighborRatio,
                                  const int radius, const Vec3 gravity, const Real k_b, const Real k_d, const Real c_s, const Real c_b,
                                  const Real dt, bool scale, const int exclude, const int antitunneling, const int itype);
void flipDeleteParticlesInObstacle(BasicParticleSystem& pts, const FlagGrid& flags);
void setFlagsFromLevelset(FlagGrid& flags, const Grid<Real>& phi, const int exclude, const int itype);
void setMACFromLevelset(MACGrid& v, const Grid<Real>& phi, const Vec3 c);

void sampleFlagsWithParticles(const FlagGrid& flags, BasicParticleSystem& parts, const int discretization, const Real randomness);
void gridParticleIndex(const BasicParticleSystem& parts, ParticleIndexSystem& indexSys, const FlagGrid& flags, Grid<int>& index, Grid<int>* counter);
void unionParticleLevelset(const BasicParticleSystem& parts, const ParticleIndexSystem& indexSys, const FlagGrid& flags, const Grid<int>& index,
                           LevelsetGrid& phi, const Real radiusFactor, const ParticleDataImpl<int>* ptype, const int exclude);
void mapPartsToMAC(const FlagGrid& flags, MACGrid& vel, MACGrid& velOld, const BasicParticleSystem& parts, const ParticleDataImpl<Vec3>& partVel,
                   Grid<Vec3>* weight, const ParticleDataImpl<int>* ptype, const int exclude);
void extrapolateMACFromWeight(MACGrid& vel, Grid<Vec3>& weight, int distance);
void markFluidCells(const BasicParticleSystem& parts, FlagGrid& flags, const Grid<Real>* phiObs, const ParticleDataImpl<int>* ptype, const int exclude);
void addGravity(const FlagGrid& flags, MACGrid& vel, Vec3 gravity, const Grid<Real>* exclude, bool scale);
void setWallBcs(const FlagGrid& flags, MACGrid& vel, const MACGrid* obvel, const MACGrid* fractions, const Grid<Real>* phiObs, int boundaryWidth);
void solvePressure(MACGrid& vel, Grid<Real>& pressure, const FlagGrid& flags, Real cgAccuracy, const Grid<Real>* phi,
                   const Grid<Real>* perCellCorr, const MACGrid* fractions, const MACGrid* obvel, Real gfClamp, Real cgMaxIterFac,
                   bool precondition, int preconditioner, bool enforceCompatibility, bool useL2Norm, bool zeroPressureFixing,
                   const Grid<Real>* curv, const Real surfTens, Grid<Real>* retRhs);
void extrapolateMACSimple(FlagGrid& flags, MACGrid& vel, int distance, LevelsetGrid* phiObs, bool intoObs);
void flipVelocityUpdate(const FlagGrid& flags, const MACGrid& vel, const MACGrid& velOld, const BasicParticleSystem& parts,
                        ParticleDataImpl<Vec3>& partVel, const Real flipRatio, const ParticleDataImpl<int>* ptype, const int exclude);
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

void load(Grid<Real>& g, const float* a) { for (IndexInt i = 0; i < g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ(); i++) g[i] = a[i]; }
void store(const Grid<Real>& g, float* a) { for (IndexInt i = 0; i < g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ(); i++) a[i] = g[i]; }
void load(FlagGrid& g, const int32_t* a) { for (IndexInt i = 0; i < g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ(); i++) g[i] = a[i]; }
void store(const FlagGrid& g, int32_t* a) { for (IndexInt i = 0; i < g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ(); i++) a[i] = g[i]; }
// Vec3 grids cross as SoA [3][n]
void load(Grid<Vec3>& g, const float* a) {
	const IndexInt n = g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ();
	for (IndexInt i = 0; i < n; i++) g[i] = Vec3(a[i], a[n + i], a[2 * n + i]);
}
void store(const Grid<Vec3>& g, float* a) {
	const IndexInt n = g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ();
	for (IndexInt i = 0; i < n; i++) {
		a[i] = g[i].x;
		a[n + i] = g[i].y;
		a[2 * n + i] = g[i].z;
	}
}

// a secondary system with the channels of the fixture cases: v_sec, l_sec, f_sec and an extra int channel; arrays are SoA with
// component stride cap.  It is filled through add(), so mDeleteChunk = np / 20 and mDeletes = 0 as after a sampling call.
struct Sec {
	BasicParticleSystem sys;
	ParticleDataImpl<Vec3> v, f;
	ParticleDataImpl<Real> l;
	ParticleDataImpl<int> x;
	Sec(FluidSolver* s) : sys(s), v(s), f(s), l(s), x(s) {
		sys.registerPdata(&v);
		sys.registerPdata(&l);
		sys.registerPdata(&f);
		sys.registerPdata(&x);
	}
	void fill(int64_t np, int64_t cap, const float* pos, const int32_t* flag, const float* pv, const float* pl, const float* pf, const int32_t* px) {
		for (int64_t i = 0; i < np; i++) {
			sys.add(BasicParticleData(Vec3(pos[i], pos[cap + i], pos[2 * cap + i])));
			sys[i].flag = flag[i];
			v[i] = Vec3(pv[i], pv[cap + i], pv[2 * cap + i]);
			f[i] = Vec3(pf[i], pf[cap + i], pf[2 * cap + i]);
			l[i] = pl[i];
			x[i] = px[i];
		}
	}
	void read(int64_t cap, int64_t* np, float* pos, int32_t* flag, float* pv, float* pl, float* pf, int32_t* px) {
		const int64_t n = sys.size();
		if (n > cap) throw std::runtime_error("secparts_record: capacity too small");
		*np = n;
		for (int64_t i = 0; i < n; i++) {
			pos[i] = sys[i].pos.x; pos[cap + i] = sys[i].pos.y; pos[2 * cap + i] = sys[i].pos.z;
			flag[i] = sys[i].flag;
			pv[i] = v[i].x; pv[cap + i] = v[i].y; pv[2 * cap + i] = v[i].z;
			pf[i] = f[i].x; pf[cap + i] = f[i].y; pf[2 * cap + i] = f[i].z;
			pl[i] = l[i];
			px[i] = x[i];
		}
	}
};

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

int rec_potentials(int sx, int sy, int sz, const int32_t* flags, const float* vel, float* normal, const float* phi, int radius,
                   const float* taus, float scale, int itype, int jtype, float* potTA, float* potWC, float* potKE, float* ratio) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid fl(&s);
	MACGrid v(&s);
	Grid<Vec3> nrm(&s);
	Grid<Real> ph(&s), ta(&s), wc(&s), ke(&s), nr(&s);
	load(fl, flags); load(v, vel); load(nrm, normal); load(ph, phi);
	load(ta, potTA); load(wc, potWC); load(ke, potKE); load(nr, ratio);
	flipComputeSecondaryParticlePotentials(ta, wc, ke, nr, fl, v, nrm, ph, radius, taus[0], taus[1], taus[2], taus[3], taus[4], taus[5], scale, itype, jtype);
	store(ta, potTA); store(wc, potWC); store(ke, potKE); store(nr, ratio); store(nrm, normal);
	REC_CATCH
}

/* `calls` sampling calls in a row on one system */
int rec_sample(const char* mode, int calls, int sx, int sy, int sz, float solver_dt, const int32_t* flags, const float* vel, const float* potTA,
               const float* potWC, const float* potKE, const float* ratio, float lMin, float lMax, float c_s, float c_b, float k_ta, float k_wc,
               float dt, int itype, int64_t np_in, int64_t cap, int64_t* np_out, float* pos, int32_t* pflag, float* pv, float* pl, float* pf,
               int32_t* px) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	s.mDt = solver_dt;
	FlagGrid fl(&s);
	MACGrid v(&s);
	Grid<Real> ta(&s), wc(&s), ke(&s), nr(&s);
	load(fl, flags); load(v, vel); load(ta, potTA); load(wc, potWC); load(ke, potKE); load(nr, ratio);
	Sec sec(&s);
	sec.fill(np_in, cap, pos, pflag, pv, pl, pf, px);
	for (int c = 0; c < calls; c++) {
		flipSampleSecondaryParticles(mode, fl, v, sec.sys, sec.v, sec.l, lMin, lMax, ta, wc, ke, nr, c_s, c_b, k_ta, k_wc, dt, itype);
		np_out[c] = sec.sys.size();
	}
	int64_t n;
	sec.read(cap, &n, pos, pflag, pv, pl, pf, px);
	REC_CATCH
}

int rec_update(const char* mode, int sx, int sy, int sz, float solver_dt, const int32_t* flags, const float* vel, const float* ratio, int radius,
               const float* gravity, float k_b, float k_d, float c_s, float c_b, float dt, int scale, int exclude, int antitunneling, int itype,
               int64_t np_in, int64_t cap, int64_t* np_out, float* pos, int32_t* pflag, float* pv, float* pl, float* pf, int32_t* px) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	s.mDt = solver_dt;
	FlagGrid fl(&s);
	MACGrid v(&s);
	Grid<Real> nr(&s);
	load(fl, flags); load(v, vel); load(nr, ratio);
	Sec sec(&s);
	sec.fill(np_in, cap, pos, pflag, pv, pl, pf, px);
	flipUpdateSecondaryParticles(mode, sec.sys, sec.v, sec.l, sec.f, fl, v, nr, radius, Vec3(gravity[0], gravity[1], gravity[2]), k_b, k_d, c_s, c_b,
	                             dt, scale != 0, exclude, antitunneling, itype);
	sec.read(cap, np_out, pos, pflag, pv, pl, pf, px);
	REC_CATCH
}

int rec_delete(int sx, int sy, int sz, const int32_t* flags, int64_t np_in, int64_t cap, int64_t* np_out, float* pos, int32_t* pflag, float* pv,
               float* pl, float* pf, int32_t* px) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid fl(&s);
	load(fl, flags);
	Sec sec(&s);
	sec.fill(np_in, cap, pos, pflag, pv, pl, pf, px);
	flipDeleteParticlesInObstacle(sec.sys, fl);
	sec.read(cap, np_out, pos, pflag, pv, pl, pf, px);
	REC_CATCH
}

int rec_set_flags(int sx, int sy, int sz, int32_t* flags, const float* phi, int exclude, int itype) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid fl(&s);
	Grid<Real> ph(&s);
	load(fl, flags); load(ph, phi);
	setFlagsFromLevelset(fl, ph, exclude, itype);
	store(fl, flags);
	REC_CATCH
}

int rec_set_mac(int sx, int sy, int sz, float* vel, const float* phi, const float* c) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	MACGrid v(&s);
	Grid<Real> ph(&s);
	load(v, vel); load(ph, phi);
	setMACFromLevelset(v, ph, Vec3(c[0], c[1], c[2]));
	store(v, vel);
	REC_CATCH
}

/* the dam break of scenes/flip01_simple.py in 3-D at res^3 with a secondary system.  par: tauMinTA, tauMaxTA, tauMinWC, tauMaxWC,
 * tauMinKE, tauMaxKE, scaleFromManta, lMin, lMax, c_s, c_b, k_ta, k_wc, k_b, k_d, gravity y of the secondary particles.
 * counts [steps][6]: live particles after the step, spawned in it, slots of the system after it (what doCompress left), live spray,
 * bubble and foam particles after it (kills of a step = live before + spawned - live after);
 * pots [4][n]: potTA, potWC, potKE, neighborRatio at the end */
int rec_loop(int res, int steps, float solver_dt, const float* par, int64_t* counts, float* pots) {
	REC_TRY
	const Vec3i gsi(res, res, res);
	const Vec3 gs(res, res, res);
	FluidSolver s(gsi, 3);
	s.mDt = solver_dt;
	FlagGrid flags(&s);
	LevelsetGrid phi(&s);
	MACGrid vel(&s), velOld(&s);
	Grid<Real> pressure(&s), potTA(&s), potWC(&s), potKE(&s), nRatio(&s);
	Grid<Vec3> tmpVec3(&s), normal(&s);
	BasicParticleSystem pp(&s);
	ParticleDataImpl<Vec3> pVel(&s);
	pp.registerPdata(&pVel);
	ParticleIndexSystem pindex(&s);
	Grid<int> gpi(&s);
	BasicParticleSystem sec(&s);
	ParticleDataImpl<Vec3> vSec(&s), fSec(&s);
	ParticleDataImpl<Real> lSec(&s);
	sec.registerPdata(&vSec);
	sec.registerPdata(&lSec);
	sec.registerPdata(&fSec);
	flags.initDomain(0, "xXyYzZ", "      ", "      ", "      ", nullptr);
	Box fluidbox(&s, Vec3::Invalid, gs * Vec3(0, 0, 0), gs * Vec3(0.4, 0.6, 1), Vec3::Invalid);
	LevelsetGrid phiInit = fluidbox.computeLevelset();
	flags.updateFromLevelset(phiInit);
	sampleFlagsWithParticles(flags, pp, 2, 0.2);
	const IndexInt n = (IndexInt)res * res * res;
	for (int t = 0; t < steps; t++) {
		pp.advectInGrid(flags, vel, 2 /* IntRK4 */, false, true, false, nullptr, 0);
		mapPartsToMAC(flags, vel, velOld, pp, pVel, &tmpVec3, nullptr, 0);
		extrapolateMACFromWeight(vel, tmpVec3, 2);
		markFluidCells(pp, flags, nullptr, nullptr, 0);
		gridParticleIndex(pp, pindex, flags, gpi, nullptr);
		unionParticleLevelset(pp, pindex, flags, gpi, phi, 1.0, nullptr, 0);
		addGravity(flags, vel, Vec3(0, -0.002, 0), nullptr, true);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		solvePressure(vel, pressure, flags, 1e-3, nullptr, nullptr, nullptr, nullptr, 1e-04, 1.5, true, 1, false, false, false, nullptr, 0., nullptr);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		extrapolateMACSimple(flags, vel, 4, nullptr, false);
		flipVelocityUpdate(flags, vel, velOld, pp, pVel, 0.97, nullptr, 0);
		flipComputeSecondaryParticlePotentials(potTA, potWC, potKE, nRatio, flags, vel, normal, phi, 2, par[0], par[1], par[2], par[3], par[4], par[5],
		                                       par[6], FlagGrid::TypeFluid, FlagGrid::TypeObstacle | FlagGrid::TypeOutflow | FlagGrid::TypeInflow);
		const int64_t before = sec.size();
		flipSampleSecondaryParticles("single", flags, vel, sec, vSec, lSec, par[7], par[8], potTA, potWC, potKE, nRatio, par[9], par[10], par[11],
		                             par[12], 0, FlagGrid::TypeFluid);
		const int64_t spawned = sec.size() - before;
		flipUpdateSecondaryParticles("linear", sec, vSec, lSec, fSec, flags, vel, nRatio, 1, Vec3(0, par[15], 0), par[13], par[14], par[9], par[10], 0,
		                             true, ParticleBase::PTRACER, 4, FlagGrid::TypeFluid);
		flipDeleteParticlesInObstacle(sec, flags);
		int64_t live2 = 0, ty[3] = {0, 0, 0};
		for (IndexInt i = 0; i < sec.size(); i++) {
			if (!sec.isActive(i)) continue;
			live2++;
			if (sec[i].flag & ParticleBase::PSPRAY) ty[0]++;
			if (sec[i].flag & ParticleBase::PBUBBLE) ty[1]++;
			if (sec[i].flag & ParticleBase::PFOAM) ty[2]++;
		}
		int64_t* c = counts + 6 * t;
		c[0] = live2;
		c[1] = spawned;
		c[2] = sec.size();
		c[3] = ty[0];
		c[4] = ty[1];
		c[5] = ty[2];
		s.step();
	}
	store(potTA, pots);
	store(potWC, pots + n);
	store(potKE, pots + 2 * n);
	store(nRatio, pots + 3 * n);
	REC_CATCH
}

}  // extern "C"
