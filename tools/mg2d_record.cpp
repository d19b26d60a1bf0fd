// mg2d_record.cpp -- the C++ side of tools/record_mg2d.py (recorder of tests/golden/mg2d.npz).  Our code: it drives the reference's
// GridMg in its 2-D mode, GridCg<ApplyMatrix2D>, solvePressure and three scene loops, and hands their state to Python.  Built
// against the build of oracle/ref.mk as tools/record_mg2d.py documents; no test builds or runs it.
//
// rec2_mg_open    GridMg(Vec3i(sx, sy, 1)), setA on the caller's three planes (Ak: a zero grid), setRhs + ONE doVCycle with
//                 setCoarsestLevelAccuracy(accuracy) and (1, 1) smoothing on the caller's rhs; the hierarchy stays open
// rec2_mg_read    one array of one level: 0 vertex types (bytes), 1 the operator as planes (3 on level 0, 5 above), 2 x, 3 b
// rec2_mg_paths   the sorted coarsening paths of level 1, 12 ints each: N.xy, U.xy, W.xy, sc, sf, inUStencil, bits of rw, bits of iw, 0
// rec2_solve      solvePressure with the multigrid preconditioner on a 2-D grid, step by step as plugin/pressure.cpp:482-523 takes
//                 them (GridCg<ApplyMatrix2D>, maxIter = 100), so that the iteration count and the system matrix are at hand.  The
//                 Python side asserts that pressure and velocity equal those of the reference's own solvePressure bit for bit.
// rec2_static_pair two PcMGStatic solves with different flags on one solver
// rec2_plume      scenes/plume_2d.py's main loop with preconditioner = PcMGDynamic
// rec2_guiding    scenes/guiding_2d.py's main loop as the scene ships it (PcMGStatic, zeroPressureFixing)
// rec2_flip       a 2-D FLIP dam break (scenes/flip02_surface.py's loop without resampling and mesh) with
//                 solvePressure(phi = phi, preconditioner = PcMGStatic) and a releaseMG after `release_after` steps
// The loops are this file's code: the same calls, the same arguments, the same order as tests/mg2d_loops.py states them for the
// package.  Shape::applyToGrid needs the Python argument store (NOPYTHON build: errMsg), so sources are applied with the shape's own
// isInsideGrid.
#include <cstdint>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

// the reference's pressure plugin as the preprocessor of oracle/ref.mk expanded it: its matrix kernels (ApplyGhostFluidDiagonal,
// CountEmptyCells, fixPressure) have no header
#include "plugin/pressure.cpp"
#include "shapes.h"
#include "particle.h"
#include "levelset.h"

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void getSpiralVelocity(const FlagGrid& flags, MACGrid& vel, Real strength, bool with3D);
void setGradientYWeight(Grid<Real>& W, const int minY, const int maxY, const Real valAtMin, const Real valAtMax);
void PD_fluid_guiding(MACGrid& vel, MACGrid& velT, Grid<Real>& pressure, FlagGrid& flags, Grid<Real>& weight, int blurRadius, Real theta, Real tau,
                      Real sigma, Real epsRel, Real epsAbs, int maxIters, Grid<Real>* phi, Grid<Real>* perCellCorr, MACGrid* fractions, MACGrid* obvel,
                      Real gfClamp, Real cgMaxIterFac, Real cgAccuracy, int preconditioner, bool zeroPressureFixing, const Grid<Real>* curv,
                      const Real surfTens);
void releaseBlurPrecomp();
void advectSemiLagrange(const FlagGrid* flags, const MACGrid* vel, GridBase* grid, int order, Real strength, int orderSpace, bool openBounds,
                        int boundaryWidth, int clampMode, int orderTrace);
void setWallBcs(const FlagGrid& flags, MACGrid& vel, const MACGrid* obvel, const MACGrid* fractions, const Grid<Real>* phiObs, int boundaryWidth);
void addBuoyancy(const FlagGrid& flags, const Grid<Real>& density, MACGrid& vel, Vec3 gravity, Real coefficient, bool scale);
void addGravity(const FlagGrid& flags, MACGrid& vel, Vec3 gravity, const Grid<Real>* exclude, bool scale);
void setOpenBound(FlagGrid& flags, int bWidth, std::string openBound, int type);
void resetOutflow(FlagGrid& flags, Grid<Real>* phi, BasicParticleSystem* parts, Grid<Real>* real, Grid<int>* index, ParticleIndexSystem* indexSys);
void sampleLevelsetWithParticles(const LevelsetGrid& phi, const FlagGrid& flags, BasicParticleSystem& parts, const int discretization, const Real randomness,
                                 const bool reset, const bool refillEmpty, const int particleFlag);
void mapPartsToMAC(const FlagGrid& flags, MACGrid& vel, MACGrid& velOld, const BasicParticleSystem& parts, const ParticleDataImpl<Vec3>& partVel,
                   Grid<Vec3>* weight, const ParticleDataImpl<int>* ptype, const int exclude);
void extrapolateMACFromWeight(MACGrid& vel, Grid<Vec3>& weight, int distance);
void extrapolateMACSimple(FlagGrid& flags, MACGrid& vel, int distance, LevelsetGrid* phiObs, bool intoObs);
void extrapolateLsSimple(Grid<Real>& phi, int distance, bool inside, bool include_walls);
void markFluidCells(const BasicParticleSystem& parts, FlagGrid& flags, const Grid<Real>* phiObs, const ParticleDataImpl<int>* ptype, const int exclude);
void gridParticleIndex(const BasicParticleSystem& parts, ParticleIndexSystem& indexSys, const FlagGrid& flags, Grid<int>& index, Grid<int>* counter);
void unionParticleLevelset(const BasicParticleSystem& parts, const ParticleIndexSystem& indexSys, const FlagGrid& flags, const Grid<int>& index,
                           LevelsetGrid& phi, const Real radiusFactor, const ParticleDataImpl<int>* ptype, const int exclude);
void flipVelocityUpdate(const FlagGrid& flags, const MACGrid& vel, const MACGrid& velOld, const BasicParticleSystem& parts,
                        ParticleDataImpl<Vec3>& partVel, const Real flipRatio, const ParticleDataImpl<int>* ptype, const int exclude);
extern int gDebugLevel;
}  // namespace Manta

using namespace Manta;

// GridMg keeps its levels private.  Explicit instantiations may name private members; each Rob<> hands one member pointer out.
namespace {
template <class Tag, class M, M ptr>
struct Rob {
	friend M get(Tag) { return ptr; }
};
typedef std::vector<std::vector<Real> > VecReal;
struct TagA { friend VecReal GridMg::*get(TagA); };
struct TagX { friend VecReal GridMg::*get(TagX); };
struct TagB { friend VecReal GridMg::*get(TagB); };
struct TagSize { friend std::vector<Vec3i> GridMg::*get(TagSize); };
}  // namespace
template struct Rob<TagA, VecReal GridMg::*, &GridMg::mA>;
template struct Rob<TagX, VecReal GridMg::*, &GridMg::mx>;
template struct Rob<TagB, VecReal GridMg::*, &GridMg::mb>;
template struct Rob<TagSize, std::vector<Vec3i> GridMg::*, &GridMg::mSize>;
// the vertex types and the coarsening paths are vectors of private types: take them through functions that never name the type
namespace {
template <class Tag, class M, M ptr>
struct RobBytes {
	friend const char* type_bytes(Tag*, const GridMg& mg, int l) { return reinterpret_cast<const char*>((mg.*ptr)[l].data()); }
};
struct TagType { };
const char* type_bytes(TagType*, const GridMg& mg, int l);
template <class Tag, class M, M ptr>
struct RobPaths {
	friend int path_dump(Tag*, const GridMg& mg, int32_t* out) {
		int n = 0;
		for (const auto& p : mg.*ptr) {
			if (out) {
				int32_t* o = out + 12 * n;
				o[0] = p.N.x; o[1] = p.N.y; o[2] = p.U.x; o[3] = p.U.y; o[4] = p.W.x; o[5] = p.W.y;
				o[6] = p.sc; o[7] = p.sf; o[8] = p.inUStencil ? 1 : 0;
				float rw = p.rw, iw = p.iw;
				memcpy(o + 9, &rw, 4);
				memcpy(o + 10, &iw, 4);
				o[11] = (p.N.z != 0 || p.U.z != 0 || p.W.z != 0) ? 1 : 0;      // every z offset is 0 in 2-D
			}
			n++;
		}
		return n;
	}
};
struct TagPaths { };
int path_dump(TagPaths*, const GridMg& mg, int32_t* out);
}  // namespace
template struct RobBytes<TagType, decltype(&GridMg::mType), &GridMg::mType>;
template struct RobPaths<TagPaths, decltype(&GridMg::mCoarseningPaths0), &GridMg::mCoarseningPaths0>;

static thread_local std::string g_err;
static std::unique_ptr<FluidSolver> g_solver;
static std::unique_ptr<GridMg> g_mg;

#define REC_TRY try {
#define REC_CATCH                \
	}                            \
	catch (std::exception & e) { \
		g_err = e.what();        \
		return 1;                \
	}                            \
	return 0;

namespace {
Grid<Real>* wrap(FluidSolver& s, const float* p) { return new Grid<Real>(&s, const_cast<float*>(p)); }
void load_mac(MACGrid& g, const float* soa, int64_t n) {
	for (int64_t i = 0; i < n; i++) g[i] = Vec3(soa[i], soa[n + i], soa[2 * n + i]);
}
void store_mac(const MACGrid& g, float* s, int64_t n) {
	for (int64_t i = 0; i < n; i++) {
		s[i] = g[i].x;
		s[n + i] = g[i].y;
		s[2 * n + i] = g[i].z;
	}
}
// iteration counts from the reference's own debug lines (pressure.cpp:442, fluidguiding.cpp:352)
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
int one_solve_count(Capture& c) {
	const std::vector<int> q = c.all("Iterations:");
	if (q.size() != 1) throw std::runtime_error("no single 'Iterations:' line from solvePressure");
	return q[0];
}
}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

int rec2_mg_close(void) {
	g_mg.reset();
	g_solver.reset();
	return 0;
}

int rec2_mg_open(int sx, int sy, const float* A0, const float* Ai, const float* Aj, const float* rhs, float accuracy, float* result, int* levels) {
	REC_TRY
	rec2_mg_close();
	g_solver.reset(new FluidSolver(Vec3i(sx, sy, 1), 2));
	FluidSolver& s = *g_solver;
	std::unique_ptr<Grid<Real> > a0(wrap(s, A0)), ai(wrap(s, Ai)), aj(wrap(s, Aj)), r(wrap(s, rhs)), d(wrap(s, result));
	Grid<Real> ak(&s);
	g_mg.reset(new GridMg(Vec3i(sx, sy, 1)));
	g_mg->setA(a0.get(), ai.get(), aj.get(), &ak);
	g_mg->setCoarsestLevelAccuracy(accuracy);
	g_mg->setSmoothing(1, 1);
	g_mg->setRhs(*r);
	g_mg->doVCycle(*d);
	*levels = (int)((*g_mg).*get(TagSize())).size();
	REC_CATCH
}

int rec2_mg_size(int level, int* size3) {
	const Vec3i& s = ((*g_mg).*get(TagSize()))[level];
	size3[0] = s.x;
	size3[1] = s.y;
	size3[2] = s.z;
	return 0;
}

int rec2_mg_read(int level, int what, void* dst) {
	const GridMg& mg = *g_mg;
	const Vec3i& s = (mg.*get(TagSize()))[level];
	const int n = s.x * s.y * s.z;
	if (what == 0) {
		memcpy(dst, type_bytes((TagType*)nullptr, mg, level), (size_t)n);
	} else if (what == 1) {
		const std::vector<Real>& A = (mg.*get(TagA()))[level];
		const int st = level == 0 ? 3 : 5;
		if ((int)A.size() != n * st) {
			g_err = "rec2_mg_read: the operator does not have 3 / 5 entries per vertex";
			return 1;
		}
		float* out = (float*)dst;
		for (int v = 0; v < n; v++)
			for (int k = 0; k < st; k++) out[(size_t)k * n + v] = A[(size_t)v * st + k];
	} else if (what == 2) {
		memcpy(dst, (mg.*get(TagX()))[level].data(), sizeof(float) * n);
	} else if (what == 3) {
		memcpy(dst, (mg.*get(TagB()))[level].data(), sizeof(float) * n);
	} else {
		g_err = "rec2_mg_read: what";
		return 1;
	}
	return 0;
}

// out == nullptr: the count only
int rec2_mg_paths(int32_t* out) { return path_dump((TagPaths*)nullptr, *g_mg, out); }

int rec2_solve(int sx, int sy, const int32_t* flags, float* vel, float* pressure, float* rhs, const float* phi, const float* fractions,
               float cgAccuracy, int useL2Norm, int zeroPressureFixing, float* A0, float* Ai, float* Aj, int* iterations) {
	REC_TRY
	const Real gfClamp = 1e-4;
	const int sz = 1;
	FluidSolver s(Vec3i(sx, sy, sz), 2);
	const int64_t n = (int64_t)sx * sy;
	FlagGrid fl(&s, const_cast<int*>(flags));
	std::unique_ptr<Grid<Real> > p(wrap(s, pressure)), r(wrap(s, rhs)), a0(wrap(s, A0)), ai(wrap(s, Ai)), aj(wrap(s, Aj));
	Grid<Real> ak(&s);
	std::unique_ptr<Grid<Real> > ph(phi ? wrap(s, phi) : nullptr);
	MACGrid v(&s), fr(&s);
	load_mac(v, vel, n);
	if (fractions) load_mac(fr, fractions, n);
	MACGrid* pfr = fractions ? &fr : nullptr;
	computePressureRhs(*r, v, *p, fl, cgAccuracy, ph.get(), nullptr, pfr, nullptr, gfClamp);
	// the system of solvePressureSystem
	MakeLaplaceMatrix(fl, *a0, *ai, *aj, ak, pfr);
	if (ph) ApplyGhostFluidDiagonal(*a0, fl, *ph, gfClamp);
	if (zeroPressureFixing || cgAccuracy < 1e-07) {
		const int numEmpty = CountEmptyCells(fl);
		IndexInt fix = -1;
		if (numEmpty == 0) {
			const Vec3i top(sx / 2, sy - 1, 0);      // pressure.cpp:357-359 (2-D: z = 0)
			for (int down = 0; down < 3 && fix < 0; down++)
				if (fl.isFluid(top - Vec3i(0, down, 0))) fix = fl.index(top - Vec3i(0, down, 0));
			for (int j = 1; j < sy - 1 && fix < 0; j++)
				for (int i = 1; i < sx - 1 && fix < 0; i++)
					if (fl.isFluid(i, j, 0)) fix = fl.index(i, j, 0);
		}
		if (fix >= 0) fixPressure(fix, Real(0), *r, *a0, *ai, *aj, ak);
	}
	{
		Grid<Real> residual(&s), search(&s), tmp(&s);
		GridCg<ApplyMatrix2D> gcg(*p, *r, residual, search, fl, tmp, a0.get(), ai.get(), aj.get(), &ak);
		gcg.setAccuracy(cgAccuracy);
		gcg.setUseL2Norm(useL2Norm != 0);
		GridMg mg(Vec3i(sx, sy, sz));
		gcg.setMGPreconditioner(GridCgInterface::PC_MGP, &mg);
		const int maxIter = 100;
		for (int iter = 0; iter < maxIter; iter++)
			if (!gcg.iterate()) iter = maxIter;
		*iterations = gcg.getIterations();
	}
	correctVelocity(v, *p, fl, cgAccuracy, ph.get(), nullptr, pfr, gfClamp);
	store_mac(v, vel, n);
	REC_CATCH
}

/* two solvePressure(preconditioner = PcMGStatic) calls on ONE solver: the second, on other flags and another velocity, is
 * preconditioned by the hierarchy the first one built (pressure.cpp:423-431) */
int rec2_static_pair(int sx, int sy, const int32_t* flagsA, float* velA, const int32_t* flagsB, float* velB, float cgAccuracy,
                     int zeroPressureFixing, int32_t* iters, float* pressureA, float* pressureB) {
	REC_TRY
	releaseMG(nullptr);
	FluidSolver s(Vec3i(sx, sy, 1), 2);
	const int64_t n = (int64_t)sx * sy;
	const int32_t* fls[2] = {flagsA, flagsB};
	float* vels[2] = {velA, velB};
	float* ps[2] = {pressureA, pressureB};
	for (int k = 0; k < 2; k++) {
		FlagGrid fl(&s, const_cast<int*>(fls[k]));
		std::unique_ptr<Grid<Real> > p(wrap(s, ps[k]));
		MACGrid v(&s);
		load_mac(v, vels[k], n);
		Capture c;
		solvePressure(v, *p, fl, cgAccuracy, nullptr, nullptr, nullptr, nullptr, 1e-04, 1.5, true, 3, false, false, zeroPressureFixing != 0, nullptr, 0.,
		              nullptr);
		iters[k] = one_solve_count(c);
		store_mac(v, vels[k], n);
	}
	releaseMG(&s);
	REC_CATCH
}

/* scenes/plume_2d.py's main loop at res x res; the fixture is recorded with preconditioner = 2 (PcMGDynamic), and with 1 (PcMIC: plain
 * CG in 2-D) the recorder holds the package's loop text against this one on the CPU checker backend */
int rec2_plume(int res, int steps, int preconditioner, int32_t* cg, float* vel_out, float* density_out, float* pressure_out) {
	REC_TRY
	const Vec3i gsi(res, res, 1);
	const Vec3 gs(res, res, 1);
	FluidSolver s(gsi, 2);
	s.mDt = 1.0;
	FlagGrid flags(&s);
	MACGrid vel(&s);
	Grid<Real> density(&s), pressure(&s);
	flags.initDomain(1, "xXyYzZ", "      ", "      ", "      ", nullptr);
	flags.fillGrid();
	setOpenBound(flags, 1, "yY", FlagGrid::TypeOutflow | FlagGrid::TypeEmpty);
	Cylinder source(&s, gs * Vec3(0.5, 0.1, 0.5), res * 0.14, gs * Vec3(0, 0.02, 0));
	for (int t = 0; t < steps; t++) {
		FOR_IJK(density) if (source.isInsideGrid(i, j, k)) density(i, j, k) = 1;
		advectSemiLagrange(&flags, &vel, &density, 2, 1.0, 1, false, -1, 2, 1);
		advectSemiLagrange(&flags, &vel, &vel, 2, 1.0, 1, false, -1, 2, 1);
		resetOutflow(flags, nullptr, nullptr, &density, nullptr, nullptr);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		addBuoyancy(flags, density, vel, Vec3(0, -4e-3, 0), 1.0, true);
		{
			Capture c;
			solvePressure(vel, pressure, flags, 1e-3, nullptr, nullptr, nullptr, nullptr, 1e-04, 1.5, true, preconditioner, false, false, false, nullptr, 0., nullptr);
			cg[t] = one_solve_count(c);
		}
		s.step();
	}
	const int64_t n = (int64_t)res * res;
	store_mac(vel, vel_out, n);
	for (int64_t i = 0; i < n; i++) {
		density_out[i] = density[i];
		pressure_out[i] = pressure[i];
	}
	REC_CATCH
}

/* scenes/guiding_2d.py's main loop at res0 * scale as the scene ships it: PcMGStatic (3), zeroPressureFixing, beta = 2, tau = 1,
 * sigma = 0.99 / tau, theta = 1, the plugin's default stop test (epsRel = epsAbs = 1e-3, maxIters = 200) */
int rec2_guiding(int res0, int scale, int steps, int32_t* pd, int32_t* cg, int cg_cap, int32_t* ncg, float* vel_out, float* density_out,
                 float* pressure_out) {
	REC_TRY
	const int res = res0 * scale;
	const Vec3i gsi(res, res, 1);
	const Vec3 gs(res, res, 1);
	releaseMG(nullptr);
	FluidSolver s(gsi, 2);
	s.mDt = 2.0 / scale;
	const double tau = 1.0, sigma = 0.99 / tau, theta = 1.0;
	FlagGrid flags(&s);
	MACGrid vel(&s), velT(&s);
	Grid<Real> density(&s), pressure(&s), W(&s);
	flags.initDomain(1, "xXyYzZ", "      ", "      ", "      ", nullptr);
	flags.fillGrid();
	Cylinder source(&s, gs * Vec3(0.5, 0.2, 0.5), gs.y * 0.14, gs * Vec3(0, 0.02 * 1.5, 0));
	getSpiralVelocity(flags, velT, 0.5 * scale, false);
	setGradientYWeight(W, 0, res / 2, 1, 1);
	setGradientYWeight(W, res / 2, res, 5, 5);
	releaseBlurPrecomp();
	*ncg = 0;
	for (int t = 0; t < steps; t++) {
		resetOutflow(flags, nullptr, nullptr, &density, nullptr, nullptr);
		FOR_IJK(density) if (source.isInsideGrid(i, j, k)) density(i, j, k) = 1;
		advectSemiLagrange(&flags, &vel, &density, 2, 1.0, 1, false, -1, 2, 1);
		advectSemiLagrange(&flags, &vel, &vel, 2, 1.0, 1, false, -1, 2, 1);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		addBuoyancy(flags, density, vel, Vec3(0, 0.25 * scale * -4e-3, 0), 1.0, true);
		{
			Capture c;
			PD_fluid_guiding(vel, velT, pressure, flags, W, 2, theta, tau, sigma, 1e-3, 1e-3, 200, nullptr, nullptr, nullptr, nullptr, 1e-04, 1.5, 1e-3, 3,
			                 true, nullptr, 0.);
			const std::vector<int> p = c.all("PD_fluid_guiding iterations:"), q = c.all("Iterations:");
			if (p.size() != 1) throw std::runtime_error("rec2_guiding: no iteration line");
			pd[t] = p[0];
			if ((int)q.size() != p[0] + 1) throw std::runtime_error("rec2_guiding: CG lines do not match the iteration count");
			for (int v : q) {
				if (*ncg >= cg_cap) throw std::runtime_error("rec2_guiding: cg_cap too small");
				cg[(*ncg)++] = v;
			}
		}
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		s.step();
	}
	releaseBlurPrecomp();
	releaseMG(&s);
	const int64_t n = (int64_t)res * res;
	store_mac(vel, vel_out, n);
	for (int64_t i = 0; i < n; i++) {
		density_out[i] = density[i];
		pressure_out[i] = pressure[i];
	}
	REC_CATCH
}

/* a 2-D FLIP dam break at res x res: the particles come from the caller (sampled by the caller's seeded generator, so that no
 * random stream has to match), the loop is flip02_surface.py's without resampling, mesh and obstacle, with
 * solvePressure(phi = phi, preconditioner = PcMGStatic) and releaseMG(solver) after `release_after` steps.
 * pos: [3][np] in and out; pvel out [3][np]. */
int rec2_flip(int res, int steps, int release_after, int preconditioner, int64_t np, float* pos, float* pvel_out, int32_t* cg, float* vel_out, float* phi_out,
              float* pressure_out, int32_t* flags_out) {
	REC_TRY
	const Vec3i gsi(res, res, 1);
	releaseMG(nullptr);      // a hierarchy that an earlier, failed call left behind is keyed by the solver's address
	FluidSolver s(gsi, 2);
	s.mDt = 0.5;
	FlagGrid flags(&s);
	MACGrid vel(&s), velOld(&s);
	Grid<Real> pressure(&s);
	Grid<Vec3> tmpVec3(&s);
	LevelsetGrid phi(&s);
	Grid<int> pindex(&s);
	BasicParticleSystem pp(&s);
	ParticleDataImpl<Vec3> pVel(&s);
	pp.registerPdata(&pVel);
	ParticleIndexSystem gpi(&s);
	flags.initDomain(0, "xXyYzZ", "      ", "      ", "      ", nullptr);
	pp.resizeAll(np);
	for (int64_t i = 0; i < np; i++) {
		pp[i].pos = Vec3(pos[i], pos[np + i], pos[2 * np + i]);
		pp[i].flag = 0;
		pVel[i] = Vec3(0.);
	}
	{
		// flip01_simple.py's breaking dam: Box(p0 = gs * (0, 0, 0), p1 = gs * (0.4, 0.6, 1)).computeLevelset(), flags.updateFromLevelset
		const Vec3 gs(res, res, 1);
		Box fluidbox(&s, Vec3::Invalid, gs * Vec3(0, 0, 0), gs * Vec3(0.4, 0.6, 1), Vec3::Invalid);
		LevelsetGrid phiInit(&s);
		fluidbox.generateLevelset(phiInit);
		flags.updateFromLevelset(phiInit);
	}
	for (int t = 0; t < steps; t++) {
		pp.advectInGrid(flags, vel, IntRK4, false, true, false, nullptr, 0);
		mapPartsToMAC(flags, vel, velOld, pp, pVel, &tmpVec3, nullptr, 0);
		extrapolateMACFromWeight(vel, tmpVec3, 2);
		markFluidCells(pp, flags, nullptr, nullptr, 0);
		gridParticleIndex(pp, gpi, flags, pindex, nullptr);
		unionParticleLevelset(pp, gpi, flags, pindex, phi, 1.0, nullptr, 0);
		extrapolateLsSimple(phi, 4, true, false);
		addGravity(flags, vel, Vec3(0, -0.002, 0), nullptr, true);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		{
			Capture c;
			solvePressure(vel, pressure, flags, 1e-3, &phi, nullptr, nullptr, nullptr, 1e-04, 1.5, true, preconditioner, false, false, false, nullptr, 0., nullptr);
			cg[t] = one_solve_count(c);
		}
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		extrapolateMACSimple(flags, vel, 1, nullptr, false);
		flipVelocityUpdate(flags, vel, velOld, pp, pVel, 0.97, nullptr, 0);
		if (t + 1 == release_after) releaseMG(&s);
		s.step();
	}
	releaseMG(&s);
	if ((int64_t)pp.size() != np) throw std::runtime_error("rec2_flip: the particle count changed");
	for (int64_t i = 0; i < np; i++) {
		pos[i] = pp[i].pos.x;
		pos[np + i] = pp[i].pos.y;
		pos[2 * np + i] = pp[i].pos.z;
		pvel_out[i] = pVel[i].x;
		pvel_out[np + i] = pVel[i].y;
		pvel_out[2 * np + i] = pVel[i].z;
	}
	const int64_t n = (int64_t)res * res;
	store_mac(vel, vel_out, n);
	for (int64_t i = 0; i < n; i++) {
		phi_out[i] = phi[i];
		pressure_out[i] = pressure[i];
		flags_out[i] = flags[i];
	}
	REC_CATCH
}

}  // extern "C"
