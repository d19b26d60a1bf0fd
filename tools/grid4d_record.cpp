/*
 * tools/grid4d_record.cpp -- the C++ half of the recorder of tests/golden/grid4d.npz (tools/record_grid4d.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid4d objects around
 * caller-owned arrays and calls the reference's own methods and plugins, all of which are in oracle/_ref/libmanta_ref.so.  Arrays
 * cross in the reference's own layout ([t][z][y][x] elements, the vector types with their components together), which is the numpy
 * bridge's.  It is compiled in a scratch directory and linked against that library.  No test runs it; nothing it is compiled with is
 * committed.
 */
#include "manta.h"
#include "grid.h"
#include "grid4d.h"
#include "particle.h"
#include "noisefield.h"
#include "shapes.h"
#include "levelset.h"
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void getComp4d(const Grid4d<Vec4>& src, Grid4d<Real>& dst, int c);
void setComp4d(const Grid4d<Real>& src, Grid4d<Vec4>& dst, int c);
Real grid4dMaxDiff(Grid4d<Real>& g1, Grid4d<Real>& g2);
Real grid4dMaxDiffInt(Grid4d<int>& g1, Grid4d<int>& g2);
Real grid4dMaxDiffVec3(Grid4d<Vec3>& g1, Grid4d<Vec3>& g2);
Real grid4dMaxDiffVec4(Grid4d<Vec4>& g1, Grid4d<Vec4>& g2);
void setRegion4d(Grid4d<Real>& dst, Vec4 start, Vec4 end, Real value);
void setRegion4dVec4(Grid4d<Vec4>& dst, Vec4 start, Vec4 end, Vec4 value);
void getSliceFrom4d(Grid4d<Real>& src, int srct, Grid<Real>& dst);
void getSliceFrom4dVec(Grid4d<Vec4>& src, int srct, Grid<Vec3>& dst, Grid<Real>* dstt);
void interpolateGrid4d(Grid4d<Real>& target, Grid4d<Real>& source, Vec4 offset, Vec4 scale, Vec4 size);
void interpolateGrid4dVec(Grid4d<Vec4>& target, Grid4d<Vec4>& source, Vec4 offset, Vec4 scale, Vec4 size);
void checkSymmetry(Grid<Real>& a, Grid<Real>* err, bool symmetrize, int axis, int bound);
void checkSymmetryVec3(Grid<Vec3>& a, Grid<Real>* err, bool symmetrize, int axis, int bound, int disable);
void testInitGridWithPos(Grid<Real>& grid);
void setNoisePdata(const BasicParticleSystem& parts, ParticleDataImpl<Real>& pd, const WaveletNoiseField& noise, Real scale);
void setNoisePdataVec3(const BasicParticleSystem& parts, ParticleDataImpl<Vec3>& pd, const WaveletNoiseField& noise, Real scale);
void setNoisePdataInt(const BasicParticleSystem& parts, ParticleDataImpl<int>& pd, const WaveletNoiseField& noise, Real scale);
void addTestParts(BasicParticleSystem& parts, int num);
void advectSemiLagrange(const FlagGrid* flags, const MACGrid* vel, GridBase* grid, int order, Real strength, int orderSpace, bool openBounds,
                        int boundaryWidth, int clampMode, int orderTrace);
void setWallBcs(const FlagGrid& flags, MACGrid& vel, const MACGrid* obvel, const MACGrid* fractions, const Grid<Real>* phiObs, int boundaryWidth);
void addBuoyancy(const FlagGrid& flags, const Grid<Real>& density, MACGrid& vel, Vec3 gravity, Real coefficient, bool scale);
void solvePressure(MACGrid& vel, Grid<Real>& pressure, const FlagGrid& flags, Real cgAccuracy, const Grid<Real>* phi,
                   const Grid<Real>* perCellCorr, const MACGrid* fractions, const MACGrid* obvel, Real gfClamp, Real cgMaxIterFac,
                   bool precondition, int preconditioner, bool enforceCompatibility, bool useL2Norm, bool zeroPressureFixing,
                   const Grid<Real>* curv, const Real surfTens, Grid<Real>* retRhs);
void sampleFlagsWithParticles(const FlagGrid& flags, BasicParticleSystem& parts, const int discretization, const Real randomness);
void mapPartsToGrid(const FlagGrid& flags, Grid<Real>& target, const BasicParticleSystem& parts, const ParticleDataImpl<Real>& source);
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

template <class T> size_t bytes(const Grid4d<T>& g) { return sizeof(T) * (size_t)g.getSizeX() * g.getSizeY() * g.getSizeZ() * g.getSizeT(); }
template <class T> void load(Grid4d<T>& g, const void* a) { memcpy(&g[0], a, bytes(g)); }
template <class T> void store(Grid4d<T>& g, void* a) { memcpy(a, &g[0], bytes(g)); }
template <class T> size_t bytes3(const Grid<T>& g) { return sizeof(T) * (size_t)g.getSizeX() * g.getSizeY() * g.getSizeZ(); }

template <class T> T value(const float* p);
template <> Real value<Real>(const float* p) { return p[0]; }
template <> int value<int>(const float* p) { return (int)p[0]; }
template <> Vec3 value<Vec3>(const float* p) { return Vec3(p[0], p[1], p[2]); }
template <> Vec4 value<Vec4>(const float* p) { return Vec4(p[0], p[1], p[2], p[3]); }

Real maxDiff(Grid4d<Real>& a, Grid4d<Real>& b) { return grid4dMaxDiff(a, b); }
Real maxDiff(Grid4d<int>& a, Grid4d<int>& b) { return grid4dMaxDiffInt(a, b); }
Real maxDiff(Grid4d<Vec3>& a, Grid4d<Vec3>& b) { return grid4dMaxDiffVec3(a, b); }
Real maxDiff(Grid4d<Vec4>& a, Grid4d<Vec4>& b) { return grid4dMaxDiffVec4(a, b); }

enum { ADD, SUB, MULT, SETCONST, ADDCONST, ADDSCALED, MULTCONST, CLAMP, GETMIN, GETMAX, GETMAXABS, MAXDIFF, SETBOUND, SETBOUNDNEUMANN };

template <class T>
void run_op(FluidSolver* s, int op, void* a, const void* b, const float* par, int ipar, float* scalar) {
	Grid4d<T> A(s), B(s);
	load(A, a);
	load(B, b);
	switch (op) {
		case ADD: A.add(B); break;
		case SUB: A.sub(B); break;
		case MULT: A.mult(B); break;
		case SETCONST: A.setConst(value<T>(par)); break;
		case ADDCONST: A.addConst(value<T>(par)); break;
		case ADDSCALED: A.addScaled(B, value<T>(par)); break;
		case MULTCONST: A.multConst(value<T>(par)); break;
		case CLAMP: A.clamp(par[0], par[1]); break;
		case GETMIN: *scalar = A.getMin(); break;
		case GETMAX: *scalar = A.getMax(); break;
		case GETMAXABS: *scalar = A.getMaxAbs(); break;
		case MAXDIFF: *scalar = maxDiff(A, B); break;
		case SETBOUND: A.setBound(value<T>(par), ipar); break;
		case SETBOUNDNEUMANN: A.setBoundNeumann(ipar); break;
		default: errMsg("unknown op");
	}
	store(A, a);
}

template <class T>
int file_io(FluidSolver* s, int write, void* a, const char* name) {
	Grid4d<T> A(s);
	load(A, a);
	const int r = write ? A.save(name) : A.load(name);
	store(A, a);
	return r;
}

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* kind 0 Real, 1 int, 2 Vec3, 3 Vec4; a is read and written, b read; par: the value / factor / clamp pair; ipar: boundaryWidth */
int rec_g4_op(int kind, int op, int sx, int sy, int sz, int st, void* a, const void* b, const float* par, int ipar, float* scalar) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), 3, st);
	if (kind == 0) run_op<Real>(&s, op, a, b, par, ipar, scalar);
	else if (kind == 1) run_op<int>(&s, op, a, b, par, ipar, scalar);
	else if (kind == 2) run_op<Vec3>(&s, op, a, b, par, ipar, scalar);
	else run_op<Vec4>(&s, op, a, b, par, ipar, scalar);
	REC_CATCH
}

/* vec != 0: setRegion4dVec4 */
int rec_g4_region(int vec, int sx, int sy, int sz, int st, void* a, const float* start, const float* end, const float* val) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), 3, st);
	if (vec) {
		Grid4d<Vec4> A(&s);
		load(A, a);
		setRegion4dVec4(A, value<Vec4>(start), value<Vec4>(end), value<Vec4>(val));
		store(A, a);
	} else {
		Grid4d<Real> A(&s);
		load(A, a);
		setRegion4d(A, value<Vec4>(start), value<Vec4>(end), val[0]);
		store(A, a);
	}
	REC_CATCH
}

/* dst (and dstt, which may be NULL) are grids of a second solver of dx x dy x dz cells */
int rec_g4_slice(int vec, int sx, int sy, int sz, int st, const void* src, int srct, int dx, int dy, int dz, void* dst, void* dstt) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), 3, st), s3(Vec3i(dx, dy, dz), 3);
	if (vec) {
		Grid4d<Vec4> A(&s);
		load(A, src);
		Grid<Vec3> D(&s3);
		Grid<Real> DT(&s3);
		memcpy(&D[0], dst, bytes3(D));
		if (dstt) memcpy(&DT[0], dstt, bytes3(DT));
		getSliceFrom4dVec(A, srct, D, dstt ? &DT : nullptr);
		memcpy(dst, &D[0], bytes3(D));
		if (dstt) memcpy(dstt, &DT[0], bytes3(DT));
	} else {
		Grid4d<Real> A(&s);
		load(A, src);
		Grid<Real> D(&s3);
		memcpy(&D[0], dst, bytes3(D));
		getSliceFrom4d(A, srct, D);
		memcpy(dst, &D[0], bytes3(D));
	}
	REC_CATCH
}

/* set == 0: getComp4d(vec4 -> real), else setComp4d(real -> vec4) */
int rec_g4_comp(int set, int sx, int sy, int sz, int st, void* vec4, void* real, int c) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), 3, st);
	Grid4d<Vec4> V(&s);
	Grid4d<Real> R(&s);
	load(V, vec4);
	load(R, real);
	if (set) setComp4d(R, V, c);
	else getComp4d(V, R, c);
	store(V, vec4);
	store(R, real);
	REC_CATCH
}

/* osz: offset, scale, size (12 floats) */
int rec_g4_interp(int vec, int tx, int ty, int tz, int tt, void* target, int sx, int sy, int sz, int st, const void* source, const float* osz) {
	REC_TRY
	FluidSolver S(Vec3i(sx, sy, sz), 3, st), T(Vec3i(tx, ty, tz), 3, tt);
	if (vec) {
		Grid4d<Vec4> src(&S), dst(&T);
		load(src, source);
		load(dst, target);
		interpolateGrid4dVec(dst, src, value<Vec4>(osz), value<Vec4>(osz + 4), value<Vec4>(osz + 8));
		store(dst, target);
	} else {
		Grid4d<Real> src(&S), dst(&T);
		load(src, source);
		load(dst, target);
		interpolateGrid4d(dst, src, value<Vec4>(osz), value<Vec4>(osz + 4), value<Vec4>(osz + 8));
		store(dst, target);
	}
	REC_CATCH
}

/* write != 0: Grid4d<T>::save(name) of a; else load(name) into a */
int rec_g4_file(int kind, int write, int sx, int sy, int sz, int st, void* a, const char* name) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), 3, st);
	int r;
	if (kind == 0) r = file_io<Real>(&s, write, a, name);
	else if (kind == 1) r = file_io<int>(&s, write, a, name);
	else if (kind == 2) r = file_io<Vec3>(&s, write, a, name);
	else r = file_io<Vec4>(&s, write, a, name);
	if (!r) errMsg("file call returned 0");
	REC_CATCH
}

/* the constructor's refusal: a Grid4d<Real> on a solver of the given dimension and fourthDim */
int rec_g4_construct(int sx, int sy, int sz, int dim, int fourthDim) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim, fourthDim);
	Grid4d<Real> A(&s);
	REC_CATCH
}

/* particle data: kind 0 Real, 1 int, 2 Vec3; a (n elements, read and written) and b live in one BasicParticleSystem of n slots;
 * t: an int channel (may be NULL where the op takes none); par: value / factor / clamp pair; ipar: flag, or begin / end in ipar, ipar2;
 * result: up to 3 words (floats, or an int for the int sum) */
}  // extern "C"

namespace {
enum { P_ADD, P_SUB, P_MULT, P_SAFEDIV, P_ADDCONST, P_ADDSCALED, P_MULTCONST, P_CLAMP, P_CLAMPMIN, P_CLAMPMAX, P_SETRANGE, P_SETFLAG, P_GETMIN,
       P_GETMAX, P_GETMAXABS, P_SUM, P_SUMFLAG, P_SUMSQUARE, P_SUMMAGNITUDE };
template <class T> void res_put(float* r, const T& v) { memcpy(r, &v, sizeof(T)); }     // a Real, an int, or the three Reals of a Vec3

template <class T>
void run_pd(FluidSolver* s, int op, int n, void* a, const void* b, const int* t, const float* par, int ipar, int ipar2, float* result) {
	BasicParticleSystem sys(s);
	ParticleDataImpl<T> A(s), B(s);
	ParticleDataImpl<int> Tt(s);
	sys.registerPdata(&A);
	sys.registerPdata(&B);
	sys.registerPdata(&Tt);
	sys.resizeAll(n);
	if (n) {
		memcpy(&A[0], a, sizeof(T) * n);
		memcpy(&B[0], b, sizeof(T) * n);
		if (t) memcpy(&Tt[0], t, sizeof(int) * n);
	}
	switch (op) {
		case P_ADD: A.add(B); break;
		case P_SUB: A.sub(B); break;
		case P_MULT: A.mult(B); break;
		case P_SAFEDIV: A.safeDiv(B); break;
		case P_ADDCONST: A.addConst(value<T>(par)); break;
		case P_ADDSCALED: A.addScaled(B, value<T>(par)); break;
		case P_MULTCONST: A.multConst(value<T>(par)); break;
		case P_CLAMP: A.clamp(par[0], par[1]); break;
		case P_CLAMPMIN: A.clampMin(par[0]); break;
		case P_CLAMPMAX: A.clampMax(par[0]); break;
		case P_SETRANGE: A.setConstRange(value<T>(par), ipar, ipar2); break;
		case P_SETFLAG: A.setConstIntFlag(value<T>(par), Tt, ipar); break;
		case P_GETMIN: result[0] = A.getMin(); break;
		case P_GETMAX: result[0] = A.getMax(); break;
		case P_GETMAXABS: result[0] = A.getMaxAbs(); break;
		case P_SUM: res_put(result, A.sum(nullptr, 0)); break;
		case P_SUMFLAG: res_put(result, A.sum(&Tt, ipar)); break;
		case P_SUMSQUARE: result[0] = A.sumSquare(); break;
		case P_SUMMAGNITUDE: result[0] = A.sumMagnitude(); break;
		default: errMsg("unknown op");
	}
	if (n) memcpy(a, &A[0], sizeof(T) * n);
}

template <class T>
int pd_file(FluidSolver* s, int write, int n, void* a, const char* name) {
	BasicParticleSystem sys(s);
	ParticleDataImpl<T> A(s);
	sys.registerPdata(&A);
	sys.resizeAll(n);
	if (n) memcpy(&A[0], a, sizeof(T) * n);
	const int r = write ? A.save(name) : A.load(name);
	const int m = (int)A.size() < n ? (int)A.size() : n;
	if (m) memcpy(a, &A[0], sizeof(T) * m);
	return r;
}
}  // namespace

extern "C" {

int rec_pd_op(int kind, int op, int n, void* a, const void* b, const int* t, const float* par, int ipar, int ipar2, float* result) {
	REC_TRY
	FluidSolver s(Vec3i(8, 8, 8), 3);
	if (kind == 0) run_pd<Real>(&s, op, n, a, b, t, par, ipar, ipar2, result);
	else if (kind == 1) run_pd<int>(&s, op, n, a, b, t, par, ipar, ipar2, result);
	else run_pd<Vec3>(&s, op, n, a, b, t, par, ipar, ipar2, result);
	REC_CATCH
}

int rec_pd_file(int kind, int write, int n, void* a, const char* name) {
	REC_TRY
	FluidSolver s(Vec3i(8, 7, 6), 3);
	int r;
	if (kind == 0) r = pd_file<Real>(&s, write, n, a, name);
	else if (kind == 1) r = pd_file<int>(&s, write, n, a, name);
	else r = pd_file<Vec3>(&s, write, n, a, name);
	if (!r) errMsg("file call returned 0");
	REC_CATCH
}

/* checkSymmetry (mac 0: a is [z][y][x]) / checkSymmetryVec3 (mac 1: a is [z][y][x][3]); err may be NULL */
int rec_symmetry(int mac, int sx, int sy, int sz, void* a, float* err, int symmetrize, int axis, int bound, int disable) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> E(&s);
	if (err) memcpy(&E[0], err, bytes3(E));
	if (mac) {
		Grid<Vec3> A(&s);
		memcpy(&A[0], a, bytes3(A));
		checkSymmetryVec3(A, err ? &E : nullptr, symmetrize != 0, axis, bound, disable);
		memcpy(a, &A[0], bytes3(A));
	} else {
		Grid<Real> A(&s);
		memcpy(&A[0], a, bytes3(A));
		checkSymmetry(A, err ? &E : nullptr, symmetrize != 0, axis, bound);
		memcpy(a, &A[0], bytes3(A));
	}
	if (err) memcpy(err, &E[0], bytes3(E));
	REC_CATCH
}

int rec_init_pos(int sx, int sy, int sz, float* grid) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Real> G(&s);
	testInitGridWithPos(G);
	memcpy(grid, &G[0], bytes3(G));
	REC_CATCH
}

/* kind 0 Real, 1 int, 2 Vec3; pos: n x 3 floats; out: n elements; the noise field of a solver of these dimensions with a fixed seed */
int rec_pd_noise(int kind, int sx, int sy, int sz, int fixedSeed, int n, const float* pos, void* out, float scale) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), 3);
	WaveletNoiseField noise(&s, fixedSeed, 0);
	BasicParticleSystem sys(&s);
	ParticleDataImpl<Real> R(&s);
	ParticleDataImpl<int> I(&s);
	ParticleDataImpl<Vec3> V(&s);
	sys.registerPdata(&R);
	sys.registerPdata(&I);
	sys.registerPdata(&V);
	sys.resizeAll(n);
	for (int i = 0; i < n; i++) sys[i].pos = Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
	if (kind == 0) { setNoisePdata(sys, R, noise, scale); memcpy(out, &R[0], sizeof(Real) * n); }
	else if (kind == 1) { setNoisePdataInt(sys, I, noise, scale); memcpy(out, &I[0], sizeof(int) * n); }
	else { setNoisePdataVec3(sys, V, noise, scale); memcpy(out, &V[0], sizeof(Vec3) * n); }
	REC_CATCH
}

/* addTestParts on a system of n0 particles with a Real channel sourced from a Real grid, a Vec3 channel sourced from a MAC grid, an
 * int channel and a Real channel without a source; every array has room for n0 + num elements and is written back at that length */
int rec_add_test_parts(int sx, int sy, int sz, int n0, int num, float* pos, int* flags, float* real, float* vec, int* ints, float* plain,
                       const float* src_real, const float* src_mac, int* size_out) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), 3);
	Grid<Real> G(&s);
	MACGrid M(&s);
	memcpy(&G[0], src_real, bytes3(G));
	memcpy(&M[0], src_mac, sizeof(Vec3) * (size_t)sx * sy * sz);
	BasicParticleSystem sys(&s);
	ParticleDataImpl<Real> R(&s), P(&s);
	ParticleDataImpl<int> I(&s);
	ParticleDataImpl<Vec3> V(&s);
	sys.registerPdata(&R);
	sys.registerPdata(&V);
	sys.registerPdata(&I);
	sys.registerPdata(&P);
	R.setSource(&G, false);
	V.setSource(&M, true);
	sys.resizeAll(n0);
	for (int i = 0; i < n0; i++) {
		sys[i].pos = Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
		sys[i].flag = flags[i];
		R[i] = real[i];
		V[i] = Vec3(vec[3 * i], vec[3 * i + 1], vec[3 * i + 2]);
		I[i] = ints[i];
		P[i] = plain[i];
	}
	addTestParts(sys, num);
	const int n = (int)sys.size();
	*size_out = n;
	for (int i = 0; i < n && i < n0 + num; i++) {
		pos[3 * i] = sys[i].pos.x; pos[3 * i + 1] = sys[i].pos.y; pos[3 * i + 2] = sys[i].pos.z;
		flags[i] = sys[i].flag;
		real[i] = R[i];
		vec[3 * i] = V[i].x; vec[3 * i + 1] = V[i].y; vec[3 * i + 2] = V[i].z;
		ints[i] = I[i];
		plain[i] = P[i];
	}
	REC_CATCH
}

}  // extern "C"

namespace {
// the iteration count of the last solve, from the reference's own debug line
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
template <class T> void out3(Grid<T>& g, void* a) { memcpy(a, &g[0], bytes3(g)); }
}  // namespace

extern "C" {

/* one pass `symms` of the loop of tools/tests/test_2005_symmAdv.py at res (2-D: res x res x 1) with `steps` advection steps per field.
 * Shape::applyToGrid is compiled out of the NOPYTHON packaging: its two kernels (shapes.cpp:41-47, 62-69) are written out here.
 * out: pressure and vel after the symmetrising, final phi and vel, final errR1, errR2, errV1, errV2; first: max of errR1, errV1 after
 * the solve */
int rec_loop_symm(int dim, int res, int steps, int symms, float* pressureSym, float* velSym, float* phiOut, float* velOut, float* errOut,
                  float* first, int* iterations) {
	REC_TRY
	const Vec3 gs(res, res, dim == 3 ? res : 1);
	FluidSolver s(Vec3i(res, res, dim == 3 ? res : 1), dim);
	s.mDt = 1.0;
	Grid<Real> errR1(&s), errV1(&s), errR2(&s), errV2(&s), rhs(&s), pressure(&s);
	FlagGrid flags(&s);
	MACGrid vel(&s);
	LevelsetGrid phi(&s);
	Sphere drop(&s, gs * Vec3(0.5, 0.5, 0.5), res * 0.25);
	const int dirsSymm[6] = {0, 2, 1, 2, 1, 0};
	const Vec3 dirsVel[6] = {Vec3(0, 2, 0), Vec3(0, -2, 0), Vec3(2, 0, 0), Vec3(-2, 0, 0), Vec3(0, 0, 2), Vec3(0, 0, -2)};
	flags.initDomain(0, "xXyYzZ", "      ", "      ", "      ", nullptr);
	vel.setConst(Vec3(0, 0, 0));
	phi.setConst(1e10);
	phi.join(drop.computeLevelset());
	const double fvOffsetZ = dim == 2 ? 1.25 : 0.0;
	flags.fillGrid();
	const int dir1 = dirsSymm[symms - (symms % 2)], dir2 = dirsSymm[symms - (symms % 2) + 1];
	const Vec3 velDir = dirsVel[symms];
	Box fluidVel(&s, Vec3::Invalid, gs * Vec3(0.30, 0.30, 0.30 - fvOffsetZ), gs * Vec3(0.70, 0.70, 0.70 + fvOffsetZ), Vec3::Invalid);
	FOR_IJK(vel) {
		if (fluidVel.isInside(Vec3(i, j + 0.5, k + 0.5))) vel(i, j, k).x = velDir.x;
		if (fluidVel.isInside(Vec3(i + 0.5, j, k + 0.5))) vel(i, j, k).y = velDir.y;
		if (fluidVel.isInside(Vec3(i + 0.5, j + 0.5, k))) vel(i, j, k).z = velDir.z;
	}
	{
		Capture cap(2);
		solvePressure(vel, pressure, flags, 1e-3, nullptr, nullptr, nullptr, nullptr, 1e-4, 99., true, 1, false, false, false, nullptr, 0., &rhs);
		*iterations = cap.iterations("Iterations:");
	}
	checkSymmetry(pressure, &errR1, false, dir1, 0);
	checkSymmetryVec3(vel, &errV1, false, dir1, 0, 0);
	first[0] = errR1.getMax();
	first[1] = errV1.getMax();
	checkSymmetry(pressure, nullptr, true, dir1, 0);
	checkSymmetryVec3(vel, nullptr, true, dir1, 0, 0);
	checkSymmetry(pressure, &errR1, false, dir1, 0);
	checkSymmetryVec3(vel, &errV1, false, dir1, 0, 0);
	if (dim == 3) {
		checkSymmetry(pressure, nullptr, true, dir2, 0);
		checkSymmetryVec3(vel, nullptr, true, dir2, 0, 0);
		checkSymmetry(pressure, &errR2, false, dir2, 0);
		checkSymmetryVec3(vel, &errV2, false, dir2, 0, 0);
	}
	out3(pressure, pressureSym);
	out3(vel, velSym);
	Box obsBox(&s, Vec3::Invalid, gs * Vec3(0.4, 0.4, 0.4 - fvOffsetZ), gs * Vec3(0.6, 0.6, 0.6 + fvOffsetZ), Vec3::Invalid);
	FOR_IJK(flags) {
		if (obsBox.isInsideGrid(i, j, k)) flags(i, j, k) = FlagGrid::TypeObstacle;
	}
	for (int t = 0; t < steps; t++) {
		checkSymmetry(phi, nullptr, true, dir1, 0);
		if (dim == 3) checkSymmetry(phi, nullptr, true, dir2, 0);
		phi.setBoundNeumann(0);
		advectSemiLagrange(&flags, &vel, &phi, 2, 1.0, 1, false, -1, 1, 1);
		checkSymmetry(phi, &errR1, false, dir1, 0);
		if (dim == 3) checkSymmetry(phi, &errR2, false, dir2, 0);
		s.step();
	}
	for (int t = 0; t < steps; t++) {
		phi.setBoundNeumann(0);
		checkSymmetryVec3(vel, nullptr, true, dir1, 0, 0);
		if (dim == 3) checkSymmetryVec3(vel, nullptr, true, dir2, 0, 0);
		advectSemiLagrange(&flags, &vel, &vel, 2, 1.0, 1, false, -1, 1, 1);
		checkSymmetryVec3(vel, &errV1, false, dir1, 0, 0);
		if (dim == 3) checkSymmetryVec3(vel, &errV2, false, dir2, 0, 0);
		s.step();
	}
	out3(phi, phiOut);
	out3(vel, velOut);
	const size_t n = (size_t)res * res * (dim == 3 ? res : 1);
	out3(errR1, errOut);
	out3(errR2, errOut + n);
	out3(errV1, errOut + 2 * n);
	out3(errV2, errOut + 3 * n);
	REC_CATCH
}

/* the generate branch of tools/tests/test_2065_partIo.py at res^3 (the noise field with a fixed seed, so that its offset does not depend
 * on the fields a process made before).  cap: room in the particle arrays.  out: the count, sampled positions, the noise channel, the
 * positions after 5 RK4 steps, the mapped density, the largest |vel| component after the solve, the CG iterations */
int rec_loop_partio(int res, int fixedSeed, int cap, int* count, float* pos0, float* pdens, float* pos1, float* densityOut, float* velMax,
                    int* iterations) {
	REC_TRY
	const Vec3 gs(res, res, res);
	FluidSolver s(Vec3i(res, res, res), 3);
	s.mDt = 0.58;
	FlagGrid flags(&s);
	MACGrid vel(&s);
	Grid<Real> pressure(&s), density(&s);
	BasicParticleSystem pp(&s);
	ParticleDataImpl<Vec3> pVel(&s);
	ParticleDataImpl<Real> pDens(&s);
	pp.registerPdata(&pVel);
	pp.registerPdata(&pDens);
	flags.initDomain(0, "xXyYzZ", "      ", "      ", "      ", nullptr);
	WaveletNoiseField noise(&s, fixedSeed, 0);
	noise.mPosScale = Vec3(100);
	noise.mClamp = true;
	noise.mClampNeg = 0;
	noise.mClampPos = 1.2;
	noise.mValScale = 0.9;
	noise.mValOffset = 0.15;
	noise.mTimeAnim = 0.1;
	Box fluidbox1(&s, Vec3::Invalid, gs * Vec3(0.2, 0.2, 0.2), gs * Vec3(0.8, 0.4, 0.8), Vec3::Invalid);
	Box fluidbox2(&s, Vec3::Invalid, gs * Vec3(0.2, 0.6, 0.2), gs * Vec3(0.8, 0.8, 0.8), Vec3::Invalid);
	{
		LevelsetGrid phiInit = fluidbox1.computeLevelset();
		phiInit.join(fluidbox2.computeLevelset());
		flags.updateFromLevelset(phiInit);
	}
	sampleFlagsWithParticles(flags, pp, 3, 0.2);
	const int n = (int)pp.size();
	*count = n;
	if (n > cap) errMsg("particle arrays too small");
	for (int i = 0; i < n; i++) { pos0[3 * i] = pp[i].pos.x; pos0[3 * i + 1] = pp[i].pos.y; pos0[3 * i + 2] = pp[i].pos.z; }
	pDens.setConst(1.3);
	flags.fillGrid();
	mapPartsToGrid(flags, density, pp, pDens);
	addBuoyancy(flags, density, vel, Vec3(0, -5e-1, 0), 1., true);
	setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
	{
		Capture cap2(2);
		solvePressure(vel, pressure, flags, 1e-3, nullptr, nullptr, nullptr, nullptr, 1e-4, 1.5, true, 1, false, false, false, nullptr, 0., nullptr);
		*iterations = cap2.iterations("Iterations:");
	}
	setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
	Real vm = 0;
	FOR_IJK(vel) { for (int c = 0; c < 3; c++) vm = std::max(vm, (Real)fabs(vel(i, j, k)[c])); }
	*velMax = vm;
	setNoisePdata(pp, pDens, noise, 1.);
	for (int i = 0; i < n; i++) pdens[i] = pDens[i];
	for (int t = 0; t < 5; t++) {
		pp.advectInGrid(flags, vel, 2 /* IntRK4 */, false, true, false, nullptr, 0);
		s.step();
	}
	if ((int)pp.size() != n) errMsg("the particle count changed");
	for (int i = 0; i < n; i++) { pos1[3 * i] = pp[i].pos.x; pos1[3 * i + 1] = pp[i].pos.y; pos1[3 * i + 2] = pp[i].pos.z; }
	density.setConst(-1.);
	mapPartsToGrid(flags, density, pp, pDens);
	out3(density, densityOut);
	REC_CATCH
}

}  // extern "C"
