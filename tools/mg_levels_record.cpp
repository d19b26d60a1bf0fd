// mg_levels_record.cpp -- the C++ side of tools/record_mg_levels.py (recorder of tests/golden/multigrid_levels.npz).  Our code: it
// drives the reference's GridMg and GridCg directly and hands their state to Python.  Built against the build of oracle/ref.mk as
// tools/record_mg_levels.py documents; no test builds or runs it.
//
// rec_mg_open     GridMg(size), setA on the caller's four planes, setRhs + ONE doVCycle with setCoarsestLevelAccuracy(accuracy)
//                 and (1, 1) smoothing on the caller's rhs; the hierarchy stays open for rec_mg_size / rec_mg_read
// rec_mg_read     one array of one level: 0 vertex types (bytes), 1 the operator as planes (4 on level 0, 14 above), 2 x, 3 b
// rec_solve       solvePressure with the multigrid preconditioner, step by step as plugin/pressure.cpp:482-523 takes them
//                 (computePressureRhs, the matrix of solvePressureSystem, GridCg with setMGPreconditioner driven as
//                 oracle/ref_shim.cpp's ref_cg_solve drives it for MIC, correctVelocity), so that the iteration count and the
//                 system matrix are at hand.  The Python side asserts that pressure, velocity and rhs equal those of the
//                 reference's own solvePressure bit for bit.
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

// the reference's pressure plugin as the preprocessor of oracle/ref.mk expanded it: its matrix kernels (ApplyGhostFluidDiagonal,
// CountEmptyCells, fixPressure) have no header
#include "plugin/pressure.cpp"

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
struct TagType;
}  // namespace
template struct Rob<TagA, VecReal GridMg::*, &GridMg::mA>;
template struct Rob<TagX, VecReal GridMg::*, &GridMg::mx>;
template struct Rob<TagB, VecReal GridMg::*, &GridMg::mb>;
template struct Rob<TagSize, std::vector<Vec3i> GridMg::*, &GridMg::mSize>;
// the vertex types are vectors of a private one-byte enum: take the member's address as bytes
namespace {
template <class Tag, class M, M ptr>
struct RobBytes {
	friend const char* type_bytes(Tag*, const GridMg& mg, int l) { return reinterpret_cast<const char*>((mg.*ptr)[l].data()); }
};
struct TagType { };
const char* type_bytes(TagType*, const GridMg& mg, int l);
}  // namespace
template struct RobBytes<TagType, decltype(&GridMg::mType), &GridMg::mType>;

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

static Grid<Real>* wrap(FluidSolver& s, const float* p) { return new Grid<Real>(&s, const_cast<float*>(p)); }
static void load_mac(MACGrid& g, const float* soa, int64_t n) {
	for (int64_t i = 0; i < n; i++) g[i] = Vec3(soa[i], soa[n + i], soa[2 * n + i]);
}

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

int rec_mg_close(void) {
	g_mg.reset();
	g_solver.reset();
	return 0;
}

int rec_mg_open(int sx, int sy, int sz, const float* A0, const float* Ai, const float* Aj, const float* Ak, const float* rhs,
                float accuracy, float* result, int* levels) {
	REC_TRY
	rec_mg_close();
	g_solver.reset(new FluidSolver(Vec3i(sx, sy, sz), 3));
	FluidSolver& s = *g_solver;
	std::unique_ptr<Grid<Real> > a0(wrap(s, A0)), ai(wrap(s, Ai)), aj(wrap(s, Aj)), ak(wrap(s, Ak)), r(wrap(s, rhs)), d(wrap(s, result));
	g_mg.reset(new GridMg(Vec3i(sx, sy, sz)));
	g_mg->setA(a0.get(), ai.get(), aj.get(), ak.get());
	g_mg->setCoarsestLevelAccuracy(accuracy);
	g_mg->setSmoothing(1, 1);
	g_mg->setRhs(*r);
	g_mg->doVCycle(*d);
	*levels = (int)((*g_mg).*get(TagSize())).size();
	REC_CATCH
}

int rec_mg_size(int level, int* size3) {
	const Vec3i& s = ((*g_mg).*get(TagSize()))[level];
	size3[0] = s.x;
	size3[1] = s.y;
	size3[2] = s.z;
	return 0;
}

int rec_mg_read(int level, int what, void* dst) {
	const GridMg& mg = *g_mg;
	const Vec3i& s = (mg.*get(TagSize()))[level];
	const int n = s.x * s.y * s.z;
	if (what == 0) {
		memcpy(dst, type_bytes((TagType*)nullptr, mg, level), (size_t)n);
	} else if (what == 1) {
		const std::vector<Real>& A = (mg.*get(TagA()))[level];
		const int st = level == 0 ? 4 : 14;
		float* out = (float*)dst;
		for (int v = 0; v < n; v++)
			for (int k = 0; k < st; k++) out[(size_t)k * n + v] = A[(size_t)v * st + k];
	} else if (what == 2) {
		memcpy(dst, (mg.*get(TagX()))[level].data(), sizeof(float) * n);
	} else if (what == 3) {
		memcpy(dst, (mg.*get(TagB()))[level].data(), sizeof(float) * n);
	} else {
		g_err = "rec_mg_read: what";
		return 1;
	}
	return 0;
}

int rec_solve(int sx, int sy, int sz, const int32_t* flags, float* vel, float* pressure, float* rhs, const float* phi,
              const float* fractions, float cgAccuracy, int useL2Norm, int zeroPressureFixing, float* A0, float* Ai, float* Aj,
              float* Ak, int* iterations) {
	REC_TRY
	const Real gfClamp = 1e-4;
	FluidSolver s(Vec3i(sx, sy, sz), 3);
	const int64_t n = (int64_t)sx * sy * sz;
	FlagGrid fl(&s, const_cast<int*>(flags));
	std::unique_ptr<Grid<Real> > p(wrap(s, pressure)), r(wrap(s, rhs)), a0(wrap(s, A0)), ai(wrap(s, Ai)), aj(wrap(s, Aj)), ak(wrap(s, Ak));
	std::unique_ptr<Grid<Real> > ph(phi ? wrap(s, phi) : nullptr);
	MACGrid v(&s), fr(&s);
	load_mac(v, vel, n);
	if (fractions) load_mac(fr, fractions, n);
	MACGrid* pfr = fractions ? &fr : nullptr;
	computePressureRhs(*r, v, *p, fl, cgAccuracy, ph.get(), nullptr, pfr, nullptr, gfClamp);
	// the system of solvePressureSystem
	MakeLaplaceMatrix(fl, *a0, *ai, *aj, *ak, pfr);
	if (ph) ApplyGhostFluidDiagonal(*a0, fl, *ph, gfClamp);
	if (zeroPressureFixing || cgAccuracy < 1e-07) {
		const int numEmpty = CountEmptyCells(fl);
		IndexInt fix = -1;
		if (numEmpty == 0) {
			const Vec3i top(sx / 2, sy - 1, sz / 2);
			for (int down = 0; down < 3 && fix < 0; down++)
				if (fl.isFluid(top - Vec3i(0, down, 0))) fix = fl.index(top - Vec3i(0, down, 0));
			for (int k = 1; k < sz - 1 && fix < 0; k++)
				for (int j = 1; j < sy - 1 && fix < 0; j++)
					for (int i = 1; i < sx - 1 && fix < 0; i++)
						if (fl.isFluid(i, j, k)) fix = fl.index(i, j, k);
		}
		if (fix >= 0) fixPressure(fix, Real(0), *r, *a0, *ai, *aj, *ak);
	}
	{
		Grid<Real> residual(&s), search(&s), tmp(&s);
		GridCg<ApplyMatrix> gcg(*p, *r, residual, search, fl, tmp, a0.get(), ai.get(), aj.get(), ak.get());
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
	for (int64_t i = 0; i < n; i++) {
		vel[i] = v[i].x;
		vel[n + i] = v[i].y;
		vel[2 * n + i] = v[i].z;
	}
	REC_CATCH
}

}  // extern "C"
