/*
 * tools/mesh_record.cpp -- the C++ half of the recorder of tests/golden/mesh.npz (tools/record_mesh.py is the other half; its header
 * has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid / Mesh objects around
 * caller-owned arrays and calls the reference's own LevelsetGrid::createMesh and Mesh methods (levelset.cpp, mesh.cpp and
 * fileio/iomeshes.cpp are part of oracle/ref.mk's library), plus the step of scenes/flip02_surface.py written against the reference's
 * classes with improvedParticleLevelset and a mesh of every step's level set.  It is compiled in a scratch directory and linked against
 * oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled with is committed.  Meshes cross as [n][3] arrays.
 */
#include "manta.h"
#include "grid.h"
#include "particle.h"
#include "levelset.h"
#include "mesh.h"
#include "shapes.h"
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <zlib.h>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void gridParticleIndex(const BasicParticleSystem& parts, ParticleIndexSystem& indexSys, const FlagGrid& flags, Grid<int>& index, Grid<int>* counter);
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

struct Quiet {
	int level;
	Quiet() : level(gDebugLevel) { gDebugLevel = 0; }
	~Quiet() { gDebugLevel = level; }
};

void fill(Mesh& m, int64_t n, const float* pos, const float* nrm, const int32_t* nflags, int64_t t, const int32_t* tris) {
	for (int64_t i = 0; i < n; i++) {
		Node nd;
		nd.pos = Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
		if (nrm) nd.normal = Vec3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
		if (nflags) nd.flags = nflags[i];
		m.addNode(nd);
	}
	for (int64_t i = 0; i < t; i++) m.addTri(Triangle(tris[3 * i], tris[3 * i + 1], tris[3 * i + 2]));
}

void drain(Mesh& m, int64_t capN, int64_t capT, int64_t* counts, float* pos, float* nrm, int32_t* tris) {
	const int64_t n = m.numNodes(), t = m.numTris();
	if (n > capN || t > capT) throw std::runtime_error("mesh_record: output arrays too small");
	counts[0] = n;
	counts[1] = t;
	for (int64_t i = 0; i < n; i++) {
		const Node& nd = m.nodes(i);
		if (nd.flags != 0) throw std::runtime_error("mesh_record: a node flag is set");
		for (int c = 0; c < 3; c++) {
			pos[3 * i + c] = nd.pos[c];
			if (nrm) nrm[3 * i + c] = nd.normal[c];
		}
	}
	for (int64_t i = 0; i < t; i++) {
		if (m.tris(i).flags != 0) throw std::runtime_error("mesh_record: a triangle flag is set");
		for (int c = 0; c < 3; c++) tris[3 * i + c] = m.tris(i).c[c];
	}
}

void load(Grid<Real>& g, const float* a) {
	const IndexInt n = g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ();
	for (IndexInt i = 0; i < n; i++) g[i] = a[i];
}

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* the mesh is given a previous content first, which createMesh has to clear */
int rec_create_mesh(int sx, int sy, int sz, const float* phi, int64_t capN, int64_t capT, int64_t* counts, float* pos, float* nrm, int32_t* tris) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	LevelsetGrid g(&s);
	load(g, phi);
	Mesh m(&s);
	m.addNode(Node(Vec3(1, 2, 3)));
	m.addTri(Triangle(0, 0, 0));
	g.createMesh(m);
	drain(m, capN, capT, counts, pos, nrm, tris);
	REC_CATCH
}

int rec_vertex_normals(int64_t n, const float* pos, int64_t t, const int32_t* tris, float* nrm) {
	REC_TRY
	FluidSolver s(Vec3i(4, 4, 4), 3);
	Mesh m(&s);
	fill(m, n, pos, nullptr, nullptr, t, tris);
	m.computeVertexNormals();
	for (int64_t i = 0; i < n; i++)
		for (int c = 0; c < 3; c++) nrm[3 * i + c] = m.nodes(i).normal[c];
	REC_CATCH
}

/* nrm holds the mesh's normals on entry and, on return, what the mesh holds after the save */
int rec_save(int sx, int sy, int sz, int64_t n, const float* pos, float* nrm, int64_t t, const int32_t* tris, const char* name) {
	REC_TRY
	Quiet q;
	FluidSolver s(Vec3i(sx, sy, sz), 3);
	Mesh m(&s);
	fill(m, n, pos, nrm, nullptr, t, tris);
	m.save(name);
	for (int64_t i = 0; i < n; i++)
		for (int c = 0; c < 3; c++) nrm[3 * i + c] = m.nodes(i).normal[c];
	REC_CATCH
}

/* load into a mesh that holds `pre` nodes at (9, 9, 9) with normal (1, 1, 1) and no triangle */
int rec_load(int sx, int sy, int sz, const char* name, int append, int pre, int64_t capN, int64_t capT, int64_t* counts, float* pos, float* nrm,
             int32_t* tris) {
	REC_TRY
	Quiet q;
	FluidSolver s(Vec3i(sx, sy, sz), 3);
	Mesh m(&s);
	for (int i = 0; i < pre; i++) {
		Node nd(Vec3(9, 9, 9));
		nd.normal = Vec3(1, 1, 1);
		m.addNode(nd);
	}
	m.load(name, append != 0);
	drain(m, capN, capT, counts, pos, nrm, tris);
	REC_CATCH
}

/* vel is SoA [3][cells]; pos [n][3] in and out */
int rec_advect(int sx, int sy, int sz, float dt, const float* vel, int64_t n, float* pos, const int32_t* nflags, int mode) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	s.mDt = dt;
	FlagGrid flags(&s);
	MACGrid v(&s);
	const IndexInt cells = (IndexInt)sx * sy * sz;
	for (IndexInt i = 0; i < cells; i++) v[i] = Vec3(vel[i], vel[cells + i], vel[2 * cells + i]);
	Mesh m(&s);
	fill(m, n, pos, nullptr, nflags, 0, nullptr);
	m.advectInGrid(flags, v, mode);
	for (int64_t i = 0; i < n; i++)
		for (int c = 0; c < 3; c++) pos[3 * i + c] = m.nodes(i).pos[c];
	REC_CATCH
}

/* op 0 scale, 1 offset, 2 rotate, 3 save_pos ; scale by (x, y, z) ; load_pos */
int rec_transform(int op, int64_t n, float* pos, float x, float y, float z) {
	REC_TRY
	FluidSolver s(Vec3i(4, 4, 4), 3);
	Mesh m(&s);
	fill(m, n, pos, nullptr, nullptr, 0, nullptr);
	if (op == 0) m.scale(Vec3(x, y, z));
	else if (op == 1) m.offset(Vec3(x, y, z));
	else if (op == 2) m.rotate(Vec3(x, y, z));
	else {
		m.save_pos();
		m.scale(Vec3(x, y, z));
		m.load_pos();
	}
	for (int64_t i = 0; i < n; i++)
		for (int c = 0; c < 3; c++) pos[3 * i + c] = m.nodes(i).pos[c];
	REC_CATCH
}

/* load_pos after the number of nodes changed: returns 1 with the reference's message */
int rec_load_pos_changed(void) {
	REC_TRY
	FluidSolver s(Vec3i(4, 4, 4), 3);
	Mesh m(&s);
	m.addNode(Node(Vec3(1, 1, 1)));
	m.save_pos();
	m.addNode(Node(Vec3(2, 2, 2)));
	m.load_pos();
	REC_CATCH
}

/* scenes/flip02_surface.py's step at res^3 (dam break, no adjustNumber) with improvedParticleLevelset in the place of
 * unionParticleLevelset; every step a copy of phi gets setBound(0, 1) and createMesh, as scenes/flip03_gen.py does it.
 * counts [steps][2], crc [steps] (crc32 of phi right after the level-set plugin); the last step's mesh; then that mesh advected
 * `advSteps` times with RK4 in the final velocity: adv [n][3] */
int rec_loop_mesh(int res, int steps, int advSteps, int64_t* counts, uint32_t* crc, int64_t capN, int64_t capT, float* pos, float* nrm, int32_t* tris,
                  float* adv) {
	REC_TRY
	Quiet q;
	const Vec3i gsi(res, res, res);
	const Vec3 gs(res, res, res);
	FluidSolver s(gsi, 3);
	s.mDt = 0.8;
	FlagGrid flags(&s);
	LevelsetGrid phi(&s), phiMesh(&s);
	MACGrid vel(&s), velOld(&s);
	Grid<Real> pressure(&s);
	Grid<Vec3> tmpVec3(&s);
	BasicParticleSystem pp(&s);
	ParticleDataImpl<Vec3> pVel(&s);
	pp.registerPdata(&pVel);
	ParticleIndexSystem pindex(&s);
	Grid<int> gpi(&s);
	Mesh mesh(&s);
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
		improvedParticleLevelset(pp, pindex, flags, gpi, phi, 1.0, 1, 1, 0.4, 3.5, nullptr, 0);
		crc[t] = (uint32_t)crc32(0L, (const Bytef*)&phi[0], (uInt)(n * sizeof(float)));
		phiMesh.copyFrom(phi);
		phiMesh.setBound(0., 1);
		phiMesh.createMesh(mesh);
		counts[2 * t] = mesh.numNodes();
		counts[2 * t + 1] = mesh.numTris();
		resetOutflow(flags, nullptr, &pp, nullptr, &gpi, &pindex);
		extrapolateLsSimple(phi, 4, true, false);
		addGravity(flags, vel, Vec3(0, -0.001, 0), nullptr, true);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		solvePressure(vel, pressure, flags, 1e-3, &phi, nullptr, nullptr, nullptr, 1e-04, 1.5, true, 1, false, false, false, nullptr, 0., nullptr);
		setWallBcs(flags, vel, nullptr, nullptr, nullptr, 0);
		extrapolateMACSimple(flags, vel, 4, nullptr, false);
		flipVelocityUpdate(flags, vel, velOld, pp, pVel, 0.97, nullptr, 0);
		s.step();
	}
	int64_t last[2];
	drain(mesh, capN, capT, last, pos, nrm, tris);
	for (int a = 0; a < advSteps; a++) mesh.advectInGrid(flags, vel, 2);
	for (int64_t i = 0; i < last[0]; i++)
		for (int c = 0; c < 3; c++) adv[3 * i + c] = mesh.nodes(i).pos[c];
	REC_CATCH
}

}  // extern "C"
