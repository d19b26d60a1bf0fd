/*
 * tools/mlflip_record.cpp -- the C++ half of the recorder of tests/golden/mlflip.npz (tools/record_mlflip.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid / BasicParticleSystem
 * objects around caller-owned arrays and calls the reference's own array copies, feature extraction and region plugins, plus the step of
 * scenes/flip01_simple.py (3-D dam break) written against the reference's classes with the per-frame calls of the MLFLIP data
 * generation beside it.  plugin/tfplugins.cpp and plugin/numpyconvert.cpp are not part of oracle/ref.mk's library and need the array
 * container of the reference's Python wrapper, which the NOPYTHON packaging lacks: the recorder's commands expand the two files with
 * the reference's `prep` into a scratch directory, and this file declares a container with the four members the plugins read and then
 * includes the two expanded files from there (-I).  Linked against oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled
 * with is committed.
 */
#include <vector>

// the element types the plugins switch on, and the container they take by value: data pointer, element type, element count, shape
enum NumpyTypes { N_INT = 0, N_FLOAT = 1, N_DOUBLE = 2, N_OTHER = 3 };
namespace Manta {
struct PyArrayContainer {
	void* pData;
	NumpyTypes DataType;
	unsigned int TotalSize;
	std::vector<long> Dims;
};
}  // namespace Manta

#include "plugin/tfplugins.cpp"        // the expanded reference sources, from the recorder's scratch directory (-I)
#include "plugin/numpyconvert.cpp"
#include "shapes.h"
#include <cstring>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void setPartType(const BasicParticleSystem& parts, ParticleDataImpl<int>& ptype, const int mark, const int stype, const FlagGrid& flags, const int cflag);
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

template <class G, class T>
void load(G& g, const T* a) {
	const IndexInt n = g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ();
	for (IndexInt i = 0; i < n; i++) g[i] = a[i];
}
template <class G, class T>
void store(const G& g, T* a) {
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

// dtype: 0 int32, 1 float32, 2 float64, anything else an element type the plugins do not know; dims: the array's shape
PyArrayContainer array_of(void* data, int dtype, int64_t total, int ndim, const int64_t* dims) {
	PyArrayContainer a;
	a.pData = data;
	a.DataType = dtype == 0 ? N_INT : dtype == 1 ? N_FLOAT : dtype == 2 ? N_DOUBLE : N_OTHER;
	a.TotalSize = (unsigned int)total;
	for (int q = 0; q < ndim; q++) a.Dims.push_back((long)dims[q]);
	return a;
}

void fill(BasicParticleSystem& sys, ParticleDataImpl<int>* pt, int64_t np, const float* pos, const int32_t* pflag, const int32_t* ptype) {
	for (int64_t i = 0; i < np; i++) {
		sys.add(BasicParticleData(Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2])));
		sys[i].flag = pflag[i];
		if (pt) (*pt)[i] = ptype[i];
	}
}

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* kind 0 Grid<Real>, 1 FlagGrid, 2 LevelsetGrid, 3 Grid<Vec3>, 4 MACGrid; grid: float / int32 [n] or float [n][3].  The grid starts
 * from what `grid` holds. */
int rec_array_to_grid(int kind, int sx, int sy, int sz, void* arr, int dtype, int64_t total, int ndim, const int64_t* dims, void* grid) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	const PyArrayContainer a = array_of(arr, dtype, total, ndim, dims);
	if (kind == 0) { Grid<Real> g(&s); load(g, (const float*)grid); copyArrayToGridReal(a, g); store(g, (float*)grid); }
	else if (kind == 1) { FlagGrid g(&s); load(g, (const int32_t*)grid); copyArrayToGridFlag(a, g); store(g, (int32_t*)grid); }
	else if (kind == 2) { LevelsetGrid g(&s); load(g, (const float*)grid); copyArrayToGridLevelset(a, g); store(g, (float*)grid); }
	else if (kind == 3) { Grid<Vec3> g(&s); load3(g, (const float*)grid); copyArrayToGridVec3(a, g); store3(g, (float*)grid); }
	else { MACGrid g(&s); load3(g, (const float*)grid); copyArrayToGridMAC(a, g); store3(g, (float*)grid); }
	REC_CATCH
}

int rec_grid_to_array(int kind, int sx, int sy, int sz, const void* grid, void* arr, int dtype, int64_t total, int ndim, const int64_t* dims) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	const PyArrayContainer a = array_of(arr, dtype, total, ndim, dims);
	if (kind == 0) { Grid<Real> g(&s); load(g, (const float*)grid); copyGridToArrayReal(g, a); }
	else if (kind == 1) { FlagGrid g(&s); load(g, (const int32_t*)grid); copyGridToArrayFlag(g, a); }
	else if (kind == 2) { LevelsetGrid g(&s); load(g, (const float*)grid); copyGridToArrayLevelset(g, a); }
	else if (kind == 3) { Grid<Vec3> g(&s); load3(g, (const float*)grid); copyGridToArrayVec3(g, a); }
	else { MACGrid g(&s); load3(g, (const float*)grid); copyGridToArrayMAC(g, a); }
	REC_CATCH
}

/* the Vec3 particle-data copies: src [n][3] -> a channel -> dst [n][3] */
int rec_pdata_vec3(int64_t n, float* src, float* dst) {
	REC_TRY
	FluidSolver s(Vec3i(8, 8, 8), 3);
	BasicParticleSystem sys(&s);
	ParticleDataImpl<Vec3> pd(&s);
	sys.registerPdata(&pd);
	for (int64_t i = 0; i < n; i++) sys.add(BasicParticleData(Vec3(0.)));
	const int64_t dims[1] = {3 * n};
	copyArrayToPdataVec3(array_of(src, 1, 3 * n, 1, dims), pd);
	copyPdataToArrayVec3(pd, array_of(dst, 1, 3 * n, 1, dims));
	REC_CATCH
}

int rec_simple(int sx, int sy, int sz, float* grid, float* arr, int64_t total, float scale) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> g(&s);
	load(g, grid);
	const int64_t dims[1] = {total};
	simpleNumpyTest(g, array_of(arr, 1, total, 1, dims), scale);
	store(g, grid);
	REC_CATCH
}

/* kind 0 vel (grid float [n][3]), 1 phi (float [n]), 2 geo (int32 [n]); pos [np][3]; ptype nullable */
int rec_feature(int kind, int sx, int sy, int sz, const void* grid, int64_t np, const float* pos, const int32_t* pflag, const int32_t* ptype,
                int exclude, int window, float scale, float* fv, int64_t fv_len, int N_row, int off_begin) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	BasicParticleSystem sys(&s);
	ParticleDataImpl<int> pt(&s);
	sys.registerPdata(&pt);
	fill(sys, &pt, np, pos, pflag, ptype ? ptype : pflag);
	const int64_t dims[1] = {fv_len};
	const PyArrayContainer a = array_of(fv, 1, fv_len, 1, dims);
	if (kind == 0) { MACGrid g(&s); load3(g, (const float*)grid); extractFeatureVel(a, N_row, off_begin, sys, g, scale, ptype ? &pt : nullptr, exclude, window); }
	else if (kind == 1) { Grid<Real> g(&s); load(g, (const float*)grid); extractFeaturePhi(a, N_row, off_begin, sys, g, scale, ptype ? &pt : nullptr, exclude, window); }
	else { FlagGrid g(&s); load(g, (const int32_t*)grid); extractFeatureGeo(a, N_row, off_begin, sys, g, scale, ptype ? &pt : nullptr, exclude, window); }
	REC_CATCH
}

/* getRegions -> r, *count; getRegionalCounts -> rcnt; extendRegion on a copy of the flags -> ext; markSmallRegions with rcnt on another
 * copy -> marked */
int rec_regions(int sx, int sy, int sz, const int32_t* flags, int ctype, int32_t* r, int32_t* count, int32_t* rcnt, int region, int exclude,
                int depth, int32_t* ext, int mark, int mexclude, int th, int32_t* marked) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid fl(&s), f2(&s), f3(&s);
	Grid<int> rr(&s), rc(&s);
	load(fl, flags); load(f2, flags); load(f3, flags);
	rr.setConst(-5);
	rc.setConst(-5);
	*count = getRegions(rr, fl, ctype);
	getRegionalCounts(rc, fl, ctype);
	extendRegion(f2, region, exclude, depth);
	markSmallRegions(f3, rc, mark, mexclude, th);
	store(rr, r); store(rc, rcnt); store(f2, ext); store(f3, marked);
	REC_CATCH
}

/* the dam break of scenes/flip01_simple.py in 3-D at res^3 and, after every step, the per-frame calls of the MLFLIP data generation on a
 * copy of the flags.  par: th, window, feature scale.  counts [steps][4]: particles, regions, labelled cells, particles whose label is
 * not 0.  At the steps snap[0] and snap[1] (counted from 1): the feature matrix fv<q> [np][N_row] (pre-filled by the caller), the labels
 * and the velocity channel [np][3] as the array copies give them; np<q> the particle count then.  The features leave out the particles
 * labelled FLUID (the layer under the surface), so some rows stay as the caller filled them. */
int rec_loop(int res, int steps, float solver_dt, const int* par, int64_t* counts, const int* snap, int64_t cap, int N_row, int64_t* np0,
             float* fv0, int32_t* lab0, float* pv0, int64_t* np1, float* fv1, int32_t* lab1, float* pv1) {
	REC_TRY
	const Vec3i gsi(res, res, res);
	const Vec3 gs(res, res, res);
	FluidSolver s(gsi, 3);
	s.mDt = solver_dt;
	FlagGrid flags(&s), work(&s);
	LevelsetGrid phi(&s);
	MACGrid vel(&s), velOld(&s);
	Grid<Real> pressure(&s);
	Grid<Vec3> tmpVec3(&s);
	Grid<int> r(&s);
	BasicParticleSystem pp(&s);
	ParticleDataImpl<Vec3> pVel(&s);
	ParticleDataImpl<int> pT(&s);
	pp.registerPdata(&pVel);
	pp.registerPdata(&pT);
	ParticleIndexSystem pindex(&s);
	Grid<int> gpi(&s);
	flags.initDomain(0, "xXyYzZ", "      ", "      ", "      ", nullptr);
	Box fluidbox(&s, Vec3::Invalid, gs * Vec3(0, 0, 0), gs * Vec3(0.4, 0.6, 1), Vec3::Invalid);
	LevelsetGrid phiInit = fluidbox.computeLevelset();
	flags.updateFromLevelset(phiInit);
	sampleFlagsWithParticles(flags, pp, 2, 0.2);
	const int th = par[0], window = par[1];
	const Real fscale = (Real)par[2] / (Real)res;
	const int FLUID = FlagGrid::TypeFluid, OBS = FlagGrid::TypeObstacle, EMPTY = FlagGrid::TypeEmpty;
	const int w = 2 * window + 1, nst = w * w * w;
	if (N_row < 5 * nst) throw std::runtime_error("mlflip_record: N_row too small");
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
		// the labelling of manta_gendata.py's save_labels, on a copy of the flags
		const int64_t np = pp.size();
		if (np > cap) throw std::runtime_error("mlflip_record: capacity too small");
		work.copyFrom(flags);
		pT.setConst(FLUID);
		const int regions = getRegions(r, work, FLUID);
		int64_t labelled = 0;
		FOR_IDX(r) { if (r[idx] > 0) labelled++; }
		getRegionalCounts(r, work, FLUID);
		markSmallRegions(work, r, EMPTY, OBS, th);
		setPartType(pp, pT, EMPTY, FLUID, work, EMPTY);
		extendRegion(work, EMPTY, OBS, 1);
		setPartType(pp, pT, 0, FLUID, work, FLUID);
		int64_t marked = 0;
		for (int64_t i = 0; i < np; i++) if (pT[i] != 0) marked++;
		int64_t* c = counts + 4 * t;
		c[0] = np; c[1] = regions; c[2] = labelled; c[3] = marked;
		for (int q = 0; q < 2; q++) {
			if (snap[q] != t + 1) continue;
			float* fv = q ? fv1 : fv0;
			int32_t* lab = q ? lab1 : lab0;
			float* pv = q ? pv1 : pv0;
			*(q ? np1 : np0) = np;
			const int64_t len = np * N_row;
			const int64_t d1[1] = {len}, d2[1] = {np}, d3[1] = {3 * np};
			const PyArrayContainer a = array_of(fv, 1, len, 1, d1);
			extractFeatureVel(a, N_row, 0, pp, vel, fscale, &pT, FLUID, window);
			extractFeaturePhi(a, N_row, 3 * nst, pp, phi, 1.0, &pT, FLUID, window);
			extractFeatureGeo(a, N_row, 4 * nst, pp, flags, 1.0, &pT, FLUID, window);
			copyPdataToArrayInt(pT, array_of(lab, 0, np, 1, d2));
			copyPdataToArrayVec3(pVel, array_of(pv, 1, 3 * np, 1, d3));
		}
		s.step();
	}
	REC_CATCH
}

}  // extern "C"
