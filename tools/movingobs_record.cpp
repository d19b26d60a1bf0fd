/*
 * tools/movingobs_record.cpp -- the C++ half of the recorder of tests/golden/movingobs.npz (tools/record_movingobs.py is the other half;
 * its header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid / shape /
 * BasicParticleSystem / MovingObstacle objects around caller-owned arrays and calls the reference's own set_wall_bcs2, setBoundMAC,
 * set_bound_MAC2, mark_surface, clear_obstacle, clamp_norm, resetPhiInObs, extrapolateMACSimple, the shapes' setters,
 * BasicParticleSystem::projectOutside and MovingObstacle::moveLinear / projectOutside, all of which are in the library of oracle/ref.mk.
 * Linked against oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled with is committed.
 *
 * The reference library is the NOPYTHON packaging, in which MovingObstacle::moveLinear throws "Not yet supported..." at its first
 * applyToGrid (movingobs.cpp:77-83): rec_move catches that and reports what had happened before it -- the shapes' new centres and the
 * reset flags.  The stamping of the shapes and the velocity pass are not reached when the obstacle has a shape.
 */
#include "manta.h"
#include "grid.h"
#include "levelset.h"
#include "movingobs.h"
#include "particle.h"
#include "shapes.h"
#include <cstring>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void set_wall_bcs2(const FlagGrid& flags, MACGrid& vel, const MACGrid& obvel);
void resetPhiInObs(const FlagGrid& flags, Grid<Real>& sdf);
void extrapolateMACSimple(FlagGrid& flags, MACGrid& vel, int distance, LevelsetGrid* phiObs, bool intoObs);
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
void fill(BasicParticleSystem& sys, int64_t np, const float* pos, const int32_t* pflag) {
	for (int64_t i = 0; i < np; i++) {
		sys.add(BasicParticleData(Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2])));
		sys[i].flag = pflag[i];
	}
}
void unfill(BasicParticleSystem& sys, int64_t np, float* pos) {
	for (int64_t i = 0; i < np; i++)
		for (int c = 0; c < 3; c++) pos[3 * i + c] = sys[i].pos[c];
}

// the protected statics and members of MovingObstacle
struct Obstacle : public MovingObstacle {
	Obstacle(FluidSolver* s, int emptyType) : MovingObstacle(s, emptyType) {}
	int id() const { return mID; }
	static void restart() { sIDcnt = 10; }
	static int counter() { return sIDcnt; }
};

// a shape from its constructor arguments: kind 0 Box (p0, p1), 1 Sphere (centre, radius, scale), 2 Cylinder (centre, radius, z)
Shape* make_shape(FluidSolver* s, int kind, const float* a) {
	if (kind == 0) return new Box(s, Vec3::Invalid, Vec3(a[0], a[1], a[2]), Vec3(a[3], a[4], a[5]));
	if (kind == 1) return new Sphere(s, Vec3(a[0], a[1], a[2]), a[3], Vec3(a[4], a[5], a[6]));
	return new Cylinder(s, Vec3(a[0], a[1], a[2]), a[3], Vec3(a[4], a[5], a[6]));
}
// what the shape holds, 8 floats: Box p0, p1 ; Sphere centre, radius ; Cylinder centre, radius, getZ() = mZ * mZDir
void shape_state(const Shape* sh, int kind, float* o) {
	for (int q = 0; q < 8; q++) o[q] = 0;
	if (kind == 0) {
		const Box* b = (const Box*)sh;
		for (int c = 0; c < 3; c++) o[c] = b->getP0()[c], o[3 + c] = b->getP1()[c];
	} else if (kind == 1) {
		const Sphere* b = (const Sphere*)sh;
		for (int c = 0; c < 3; c++) o[c] = b->getCenter()[c];
		o[3] = b->getRadius();
	} else {
		const Cylinder* b = (const Cylinder*)sh;
		for (int c = 0; c < 3; c++) o[c] = b->getCenter()[c], o[4 + c] = b->getZ()[c];
		o[3] = b->getRadius();
	}
}

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

int rec_set_wall_bcs2(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* obvel) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid f(&s);
	MACGrid v(&s), o(&s);
	load(f, flags); load3(v, vel); load3(o, obvel);
	set_wall_bcs2(f, v, o);
	store3(v, vel);
	REC_CATCH
}

/* rule 0 setBoundMAC(normalOnly = false), 1 setBoundMAC(normalOnly = true), 2 set_bound_MAC2 */
int rec_set_bound_mac(int sx, int sy, int sz, float* vel, float vx, float vy, float vz, int w, int rule) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	MACGrid v(&s);
	load3(v, vel);
	if (rule == 2) v.set_bound_MAC2(Vec3(vx, vy, vz), w);
	else v.setBoundMAC(Vec3(vx, vy, vz), w, rule == 1);
	store3(v, vel);
	REC_CATCH
}

/* mark_surface keeps its neighbour list in a function static that the FIRST call of a process fills for its solver's dimension
 * (grid.cpp:932): one process records 3-D grids only, or 2-D grids only */
int rec_mark_surface(int sx, int sy, int sz, int32_t* flags) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid f(&s);
	load(f, flags);
	f.mark_surface();
	store(f, flags);
	REC_CATCH
}

int rec_clear_obstacle(int sx, int sy, int sz, int32_t* flags, int include_boundary) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid f(&s);
	load(f, flags);
	f.clear_obstacle(include_boundary != 0);
	store(f, flags);
	REC_CATCH
}

/* kind 0 Grid<Real>, 1 Grid<Vec3>, 2 MACGrid */
int rec_clamp_norm(int kind, int sx, int sy, int sz, float* data, float val) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	if (kind == 0) { Grid<Real> g(&s); load(g, data); g.clamp_norm(val); store(g, data); }
	else if (kind == 1) { Grid<Vec3> g(&s); load3(g, data); g.clamp_norm(val); store3(g, data); }
	else { MACGrid g(&s); load3(g, data); g.clamp_norm(val); store3(g, data); }
	REC_CATCH
}

int rec_reset_phi_in_obs(int sx, int sy, int sz, const int32_t* flags, float* sdf) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid f(&s);
	Grid<Real> g(&s);
	load(f, flags); load(g, sdf);
	resetPhiInObs(f, g);
	store(g, sdf);
	REC_CATCH
}

/* phi nullable */
int rec_extrapolate(int sx, int sy, int sz, const int32_t* flags, float* vel, int distance, const float* phi, int intoObs) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid f(&s);
	MACGrid v(&s);
	LevelsetGrid p(&s);
	load(f, flags); load3(v, vel);
	if (phi) load(p, phi);
	extrapolateMACSimple(f, v, distance, phi ? &p : nullptr, intoObs != 0);
	store3(v, vel);
	REC_CATCH
}

/* the shapes' setters: the shape of (kind, args) after setCenter(centre) and, for a cylinder with doCyl != 0, setRadius(r) and setZ(z);
 * state: 8 floats (shape_state), centre3: getCenter() */
int rec_shape_setters(int kind, const float* args, const float* centre, int doCyl, float r, const float* z, float* state, float* centre3) {
	REC_TRY
	FluidSolver s(Vec3i(8, 8, 8), 3);
	Shape* sh = make_shape(&s, kind, args);
	sh->setCenter(Vec3(centre[0], centre[1], centre[2]));
	if (kind == 2 && doCyl) {
		((Cylinder*)sh)->setRadius(r);
		((Cylinder*)sh)->setZ(Vec3(z[0], z[1], z[2]));
	}
	shape_state(sh, kind, state);
	const Vec3 c = sh->getCenter();
	for (int q = 0; q < 3; q++) centre3[q] = c[q];
	delete sh;
	REC_CATCH
}

/* ids[q] = the ID of the q-th MovingObstacle of a fresh counter, q < count; *threw = the index of the construction that threw (-1:
 * none), message: its text (256 bytes); *after = the counter afterwards.  The counter is put back to 10 before and after. */
int rec_ids(int count, int32_t* ids, int* threw, char* message, int* after) {
	REC_TRY
	FluidSolver s(Vec3i(8, 8, 8), 3);
	Obstacle::restart();
	*threw = -1;
	message[0] = 0;
	for (int q = 0; q < count; q++) {
		ids[q] = 0;
		try {
			Obstacle o(&s, FlagGrid::TypeEmpty);
			ids[q] = o.id();
		} catch (std::exception& e) {
			if (*threw < 0) {
				*threw = q;
				strncpy(message, e.what(), 255);
				message[255] = 0;
			}
		}
	}
	*after = Obstacle::counter();
	Obstacle::restart();
	REC_CATCH
}

/* MovingObstacle number `which` (0 .. 4) of a fresh counter, with emptyType and nshapes shapes (kinds, args: 8 floats each), then
 * moveLinear(t, t0, t1, p0, p1, flags, vel, smooth) on a solver whose time step is dt.  *threw = 1 when moveLinear threw (message: its
 * text); flags, vel and states ([nshapes][8]) are what the call left in either case. */
int rec_move(int sx, int sy, int sz, float dt, int which, int emptyType, int nshapes, const int32_t* kinds, const float* args, float t, float t0,
             float t1, const float* p0, const float* p1, int smooth, int32_t* flags, float* vel, float* states, int* threw, char* message) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	s.mDt = dt;
	FlagGrid f(&s);
	MACGrid v(&s);
	load(f, flags); load3(v, vel);
	Obstacle::restart();
	for (int q = 0; q < which; q++) Obstacle burn(&s, FlagGrid::TypeEmpty);
	Obstacle o(&s, emptyType);
	Obstacle::restart();
	std::vector<Shape*> shapes;
	for (int q = 0; q < nshapes; q++) {
		shapes.push_back(make_shape(&s, kinds[q], args + 8 * q));
		o.add(shapes.back());
	}
	*threw = 0;
	message[0] = 0;
	try {
		o.moveLinear(t, t0, t1, Vec3(p0[0], p0[1], p0[2]), Vec3(p1[0], p1[1], p1[2]), f, v, smooth != 0);
	} catch (std::exception& e) {
		*threw = 1;
		strncpy(message, e.what(), 255);
		message[255] = 0;
	}
	store(f, flags); store3(v, vel);
	for (int q = 0; q < nshapes; q++) {
		shape_state(shapes[q], kinds[q], states + 8 * q);
		delete shapes[q];
	}
	REC_CATCH
}

/* BasicParticleSystem::projectOutside(gradient): pos [np][3] in and out.  The random stream is a function static of the reference:
 * it goes on from call to call for the life of the process. */
int rec_project(int sx, int sy, int sz, const float* gradient, int64_t np, float* pos, const int32_t* pflag) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	Grid<Vec3> g(&s);
	load3(g, gradient);
	BasicParticleSystem sys(&s);
	fill(sys, np, pos, pflag);
	sys.projectOutside(g);
	unfill(sys, np, pos);
	REC_CATCH
}

/* MovingObstacle::projectOutside(flags, parts): the same stream */
int rec_obstacle_project(int sx, int sy, int sz, const int32_t* flags, int64_t np, float* pos, const int32_t* pflag) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), sz > 1 ? 3 : 2);
	FlagGrid f(&s);
	load(f, flags);
	BasicParticleSystem sys(&s);
	fill(sys, np, pos, pflag);
	Obstacle::restart();
	Obstacle o(&s, FlagGrid::TypeEmpty);
	Obstacle::restart();
	o.projectOutside(f, sys);
	unfill(sys, np, pos);
	REC_CATCH
}

}  // extern "C"
