/*
 * tools/vsheet_record.cpp -- the C++ half of the recorder of tests/golden/vsheet.npz (tools/record_vsheet.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / VortexSheetMesh / MACGrid
 * objects around caller-owned arrays and calls the reference's own calcVorticity, reinitTexCoords, meshSmokeInflow, vorticitySource,
 * smoothVorticity, texcoordInflow and advectInGrid.  plugin/vortexplugins.cpp is not part of oracle/ref.mk's library and is expanded
 * into a scratch directory and compiled next to this file.  Linked against oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is
 * compiled with is committed.
 */
#include "manta.h"
#include "grid.h"
#include "mesh.h"
#include "shapes.h"
#include "vortexsheet.h"
#include "commonkernels.h"
#include <iostream>
#include <sstream>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void texcoordInflow(VortexSheetMesh& mesh, const Shape* shape, const MACGrid& vel);
void meshSmokeInflow(VortexSheetMesh& mesh, const Shape* shape, Real amount);
void vorticitySource(VortexSheetMesh& mesh, Vec3 gravity, const MACGrid* vel, const MACGrid* velOld, Real scale, Real maxAmount, Real mult);
void smoothVorticity(VortexSheetMesh& mesh, int iter, Real sigma, Real alpha);
void VICintegration(VortexSheetMesh& mesh, Real sigma, Grid<Vec3>& vel, const FlagGrid& flags, Grid<Vec3>* vorticity, Real cgMaxIterFac, Real cgAccuracy,
                    Real scale, int precondition);
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

// the reference offset is a protected member without a getter
struct Sheet : public VortexSheetMesh {
	Sheet(FluidSolver* s) : VortexSheetMesh(s) {}
	Vec3 offset() const { return mTexOffset; }
	void sizeChannels() { rebuildChannels(); }      // what rebuildCorners() ends with: resize() of every channel, new entries T()
};

std::unique_ptr<FluidSolver> g_solver;
std::unique_ptr<Sheet> g_mesh;

std::unique_ptr<Shape> make_shape(int kind, const float* a, const float* b) {
	FluidSolver* s = g_solver.get();
	if (kind == 0) return std::unique_ptr<Shape>(new Box(s, Vec3::Invalid, Vec3(a[0], a[1], a[2]), Vec3(b[0], b[1], b[2]), Vec3::Invalid));
	return std::unique_ptr<Shape>(new Sphere(s, Vec3(a[0], a[1], a[2]), b[0], Vec3(1, 1, 1)));
}
void fill_mac(MACGrid& g, const float* soa) {
	const IndexInt n = (IndexInt)g.getSizeX() * g.getSizeY() * g.getSizeZ();
	for (IndexInt i = 0; i < n; i++) g[i] = Vec3(soa[i], soa[n + i], soa[2 * n + i]);
}
void put3(float* out, int64_t i, const Vec3& v) {
	for (int c = 0; c < 3; c++) out[3 * i + c] = v[c];
}
Vec3 get3(const float* in, int64_t i) { return Vec3(in[3 * i], in[3 * i + 1], in[3 * i + 2]); }

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* a solver and a sheet: clear(), then addNode / addTri per row; rebuildCorners() sizes the channels (rebuildChannels).  opposite (nullable): the corner
 * table to install with addCorner (rebuildCorners() refuses a mesh with boundary edges); without it rebuildCorners() runs */
int rec_open(int sx, int sy, int sz, float dt, int64_t nn, const float* pos, const int32_t* nflags, int64_t nt, const int32_t* tris,
             const int32_t* opposite) {
	REC_TRY
	g_mesh.reset();
	g_solver.reset(new FluidSolver(Vec3i(sx, sy, sz), 3));
	g_solver->mDt = dt;
	g_mesh.reset(new Sheet(g_solver.get()));
	Sheet& m = *g_mesh;
	m.clear();
	for (int64_t i = 0; i < nn; i++) {
		m.addNode(Node(get3(pos, i)));
		m.nodes(i).flags = nflags[i];
	}
	for (int64_t t = 0; t < nt; t++) m.addTri(Triangle(tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]));
	if (opposite) {
		for (int64_t t = 0; t < nt; t++)
			for (int c = 0; c < 3; c++) {
				Corner k((int)t, tris[3 * t + c]);
				k.next = (int)(3 * t + (c + 1) % 3);
				k.prev = (int)(3 * t + (c + 2) % 3);
				k.opposite = opposite[3 * t + c];
				m.addCorner(k);
			}
		m.sizeChannels();
	} else if (nt) {
		m.rebuildCorners();
	}
	REC_CATCH
}
int rec_close(void) {
	REC_TRY
	g_mesh.reset();
	g_solver.reset();
	REC_CATCH
}
int rec_corners(int32_t* opposite) {
	REC_TRY
	for (int c = 0; c < 3 * g_mesh->numTris(); c++) opposite[c] = g_mesh->corners(c).opposite;
	REC_CATCH
}

/* every pointer nullable */
int rec_set(const float* vort, const float* smoothed, const float* circ, const float* smoke, const float* particles) {
	REC_TRY
	Sheet& m = *g_mesh;
	for (int t = 0; t < m.numTris(); t++) {
		VortexSheetInfo& v = m.sheet(t);
		if (vort) v.vorticity = get3(vort, t);
		if (smoothed) v.vorticitySmoothed = get3(smoothed, t);
		if (circ) v.circulation = get3(circ, t);
		if (smoke) v.smokeAmount = smoke[t];
		if (particles) v.smokeParticles = particles[t];
	}
	REC_CATCH
}
int rec_get(float* vort, float* smoothed, float* circ, float* smoke, float* particles, float* tex1, float* tex2, float* turb, float* pos) {
	REC_TRY
	Sheet& m = *g_mesh;
	for (int t = 0; t < m.numTris(); t++) {
		const VortexSheetInfo& v = m.sheet(t);
		put3(vort, t, v.vorticity);
		put3(smoothed, t, v.vorticitySmoothed);
		put3(circ, t, v.circulation);
		smoke[t] = v.smokeAmount;
		particles[t] = v.smokeParticles;
	}
	for (int i = 0; i < m.numNodes(); i++) {
		put3(tex1, i, m.tex1(i));
		put3(tex2, i, m.tex2(i));
		turb[2 * i] = m.turb(i).k;
		turb[2 * i + 1] = m.turb(i).epsilon;
		put3(pos, i, m.nodes(i).pos);
	}
	REC_CATCH
}
int rec_offset(float* out) {
	REC_TRY
	const Vec3 o = g_mesh->offset();
	for (int c = 0; c < 3; c++) out[c] = o[c];
	REC_CATCH
}

int rec_calc_vorticity(void) {
	REC_TRY
	g_mesh->calcVorticity();
	REC_CATCH
}
int rec_reinit_tex(void) {
	REC_TRY
	g_mesh->reinitTexCoords();
	REC_CATCH
}
int rec_smoke_inflow(int kind, const float* a, const float* b, float amount) {
	REC_TRY
	std::unique_ptr<Shape> sh = make_shape(kind, a, b);
	meshSmokeInflow(*g_mesh, sh.get(), amount);
	REC_CATCH
}
/* vel, velOld: [3][n] planes, or both null */
int rec_source(const float* gravity, const float* vel, const float* velOld, float scale, float maxAmount, float mult) {
	REC_TRY
	const Vec3 g(gravity[0], gravity[1], gravity[2]);
	if (vel) {
		MACGrid v1(g_solver.get()), v0(g_solver.get());
		fill_mac(v1, vel);
		fill_mac(v0, velOld);
		vorticitySource(*g_mesh, g, &v1, &v0, scale, maxAmount, mult);
	} else {
		vorticitySource(*g_mesh, g, nullptr, nullptr, scale, maxAmount, mult);
	}
	REC_CATCH
}
int rec_smooth(int iter, float sigma, float alpha) {
	REC_TRY
	smoothVorticity(*g_mesh, iter, sigma, alpha);
	REC_CATCH
}
/* the table smoothVorticity builds inside itself, formed from the reference's own getFaceCenter, normSquare and the float exp, with
 * the plugin's `const Real mult = -0.5 / sigma / sigma`; record_vsheet.py proves it is the plugin's by reproducing the plugin's output
 * from it bit for bit */
int rec_smooth_table(float sigma_in, float* weights, int32_t* index) {
	REC_TRY
	Sheet& m = *g_mesh;
	const Real sigma = sigma_in;
	const Real mult = -0.5 / sigma / sigma;
	for (int i = 0; i < m.numTris(); i++)
		for (int c = 0; c < 3; c++) {
			const int oc = m.corners(i, c).opposite;
			if (oc >= 0) {
				const int t = m.corners(oc).tri;
				weights[3 * i + c] = std::exp(normSquare(m.getFaceCenter(t) - m.getFaceCenter(i)) * mult);
				index[3 * i + c] = t;
			} else {
				weights[3 * i + c] = 0;
				index[3 * i + c] = 0;
			}
		}
	REC_CATCH
}
int rec_inflow(int kind, const float* a, const float* b, const float* vel) {
	REC_TRY
	std::unique_ptr<Shape> sh = make_shape(kind, a, b);
	MACGrid v(g_solver.get());
	fill_mac(v, vel);
	texcoordInflow(*g_mesh, sh.get(), v);
	REC_CATCH
}
int rec_advect(const int32_t* flags, const float* vel, int mode) {
	REC_TRY
	FlagGrid fl(g_solver.get());
	MACGrid v(g_solver.get());
	const IndexInt n = (IndexInt)fl.getSizeX() * fl.getSizeY() * fl.getSizeZ();
	for (IndexInt i = 0; i < n; i++) fl[i] = flags[i];
	fill_mac(v, vel);
	g_mesh->advectInGrid(fl, v, mode);
	REC_CATCH
}

/* VICintegration on a MAC (mac != 0) or Vec3 velocity grid.  flags[n]; out: vort[3][n], vel[3][n] (planes), rhs[3][n] -- the right-hand
 * sides, formed here from the plugin's vort with the reference's own CurlOp and GetShiftedComponent / GetComponent on one reused grid,
 * as the plugin forms them -- and iterations[3], read from the line the plugin prints per component */
int rec_vic(float sigma, const int32_t* flags, int mac, float cgMaxIterFac, float cgAccuracy, float scale, int precondition, float* vort_out,
            float* vel_out, float* rhs_out, int32_t* iterations) {
	REC_TRY
	FluidSolver* s = g_solver.get();
	FlagGrid fl(s);
	const IndexInt n = (IndexInt)fl.getSizeX() * fl.getSizeY() * fl.getSizeZ();
	for (IndexInt i = 0; i < n; i++) fl[i] = flags[i];
	Grid<Vec3> vort(s);
	MACGrid vm(s);
	Grid<Vec3> vc(s);
	Grid<Vec3>& vel = mac ? (Grid<Vec3>&)vm : vc;
	std::ostringstream captured;
	std::streambuf* old = std::cout.rdbuf(captured.rdbuf());
	try {
		VICintegration(*g_mesh, sigma, vel, fl, &vort, cgMaxIterFac, cgAccuracy, scale, precondition);
	} catch (...) {
		std::cout.rdbuf(old);
		throw;
	}
	std::cout.rdbuf(old);
	const std::string text = captured.str();
	size_t at = 0;
	for (int c = 0; c < 3; c++) {
		at = text.find("CG iterations:", at);
		if (at == std::string::npos) throw std::runtime_error("vsheet_record: no iteration count in the plugin's output");
		at += 14;
		iterations[c] = atoi(text.c_str() + at);
	}
	Grid<Vec3> curl(s);
	Grid<Real> rhs(s);
	CurlOp(vort, curl);
	for (int c = 0; c < 3; c++) {
		if (mac) GetShiftedComponent(curl, rhs, c);
		else GetComponent(curl, rhs, c);
		for (IndexInt i = 0; i < n; i++) rhs_out[c * n + i] = rhs[i];
	}
	for (IndexInt i = 0; i < n; i++)
		for (int c = 0; c < 3; c++) {
			vort_out[c * n + i] = vort[i][c];
			vel_out[c * n + i] = vel[i][c];
		}
	REC_CATCH
}

}  // extern "C"
