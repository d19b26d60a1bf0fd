/*
 * tools/meshops_record.cpp -- the C++ half of the recorder of tests/golden/meshops.npz (tools/record_meshops.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Mesh objects around
 * caller-owned arrays and calls the reference's own Mesh::rebuildCorners / rebuildLookup, smoothMesh and killSmallComponents
 * (plugin/meshplugins.cpp, expanded by the reference's `prep` into a scratch directory and compiled with this file).  It is linked
 * against oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled with is committed.  Meshes cross as [n][3] arrays.
 */
#include "manta.h"
#include "grid.h"
#include "levelset.h"
#include "mesh.h"
#include <chrono>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void smoothMesh(Mesh& mesh, Real strength, int steps, Real minLength);
void killSmallComponents(Mesh& mesh, int elements);
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

void fill(Mesh& m, int64_t n, const float* pos, const float* nrm, const int32_t* nflags, int64_t t, const int32_t* tris, const int32_t* tflags) {
	for (int64_t i = 0; i < n; i++) {
		Node nd;
		nd.pos = Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
		if (nrm) nd.normal = Vec3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
		if (nflags) nd.flags = nflags[i];
		m.addNode(nd);
	}
	for (int64_t i = 0; i < t; i++) {
		Triangle tr(tris[3 * i], tris[3 * i + 1], tris[3 * i + 2]);
		if (tflags) tr.flags = tflags[i];
		m.addTri(tr);
	}
}

// the 1-ring lookup as two CSR tables (std::set iterates ascending)
void rings(Mesh& m, int32_t* nodeOff, int32_t* nodes, int32_t* triOff, int32_t* tris, int64_t cap) {
	int64_t a = 0, b = 0;
	for (int i = 0; i < m.numNodes(); i++) {
		nodeOff[i] = (int32_t)a;
		triOff[i] = (int32_t)b;
		OneRing& r = m.get1Ring(i);
		if ((int64_t)(a + r.nodes.size()) > cap || (int64_t)(b + r.tris.size()) > cap) throw std::runtime_error("meshops_record: ring arrays too small");
		for (std::set<int>::iterator it = r.nodes.begin(); it != r.nodes.end(); ++it) nodes[a++] = *it;
		for (std::set<int>::iterator it = r.tris.begin(); it != r.tris.end(); ++it) tris[b++] = *it;
	}
	nodeOff[m.numNodes()] = (int32_t)a;
	triOff[m.numNodes()] = (int32_t)b;
}

// the four sums of Mesh::computeCenterOfMass before its division, one triangle after the other, from the mesh's float positions
void serial_sums(Mesh& m, double* out) {
	double s[4] = {0, 0, 0, 0};
	for (int t = 0; t < m.numTris(); t++) {
		double p[3][3];
		for (int k = 0; k < 3; k++)
			for (int c = 0; c < 3; c++) p[k][c] = (double)m.getNode(t, k)[c];
		const double cx = p[0][1] * p[1][2] - p[0][2] * p[1][1], cy = p[0][2] * p[1][0] - p[0][0] * p[1][2], cz = p[0][0] * p[1][1] - p[0][1] * p[1][0];
		const double cvol = (cx * p[2][0] + cy * p[2][1] + cz * p[2][2]) / 6.0;
		s[0] += cvol;
		for (int c = 0; c < 3; c++) s[1 + c] += ((p[0][c] + p[1][c]) + p[2][c]) * (cvol / 4.0);
	}
	memcpy(out, s, sizeof(s));
}

struct CoutCapture {
	std::ostringstream text;
	std::streambuf* old;
	CoutCapture() : old(std::cout.rdbuf(text.rdbuf())) {}
	~CoutCapture() { std::cout.rdbuf(old); }
};

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* opposite[3t]; the lookup as addTri maintained it must equal the lookup rebuildLookup() builds from the corners */
int rec_connectivity(int64_t n, const float* pos, int64_t t, const int32_t* tris, int32_t* opposite, int32_t* nodeOff, int32_t* nodes,
                     int32_t* triOff, int32_t* rtris, int64_t cap, double* seconds) {
	REC_TRY
	FluidSolver s(Vec3i(8, 8, 8), 3);
	Mesh m(&s);
	fill(m, n, pos, nullptr, nullptr, t, tris, nullptr);
	std::vector<int32_t> a(n + 1), b(cap), c(n + 1), d(cap);
	rings(m, a.data(), b.data(), c.data(), d.data(), cap);
	const double t0 = now();
	m.rebuildCorners();
	m.rebuildLookup();
	if (seconds) *seconds = now() - t0;
	for (int64_t i = 0; i < 3 * t; i++) {
		const Corner& k = m.corners((int)i);
		if (k.tri != i / 3 || k.node != tris[i] || k.next != 3 * (i / 3) + (i + 1) % 3 || k.prev != 3 * (i / 3) + (i + 2) % 3)
			throw std::runtime_error("meshops_record: corner numbering differs");
		opposite[i] = k.opposite;
	}
	rings(m, nodeOff, nodes, triOff, rtris, cap);
	if (memcmp(a.data(), nodeOff, 4 * (n + 1)) || memcmp(c.data(), triOff, 4 * (n + 1)) || memcmp(b.data(), nodes, 4 * nodeOff[n]) ||
	    memcmp(d.data(), rtris, 4 * triOff[n]))
		throw std::runtime_error("meshops_record: rebuildLookup differs from the lookup addTri maintained");
	REC_CATCH
}

/* sums[4]: our serial restatement of the four sums of computeCenterOfMass before the steps (the reference keeps only their quotients,
 * and the positions between the steps and the rescale do not leave the plugin: the final positions are what pins the second four) */
int rec_smooth(float dt, int64_t n, float* pos, const int32_t* nflags, int64_t t, const int32_t* tris, float strength, int steps, float minLength,
               double* sums, double* seconds) {
	REC_TRY
	FluidSolver s(Vec3i(8, 8, 8), 3);
	s.mDt = dt;
	Mesh m(&s);
	fill(m, n, pos, nullptr, nflags, t, tris, nullptr);
	serial_sums(m, sums);
	const double t0 = now();
	smoothMesh(m, strength, steps, minLength);
	if (seconds) *seconds = now() - t0;
	for (int64_t i = 0; i < n; i++)
		for (int c = 0; c < 3; c++) pos[3 * i + c] = m.nodes(i).pos[c];
	if (m.numNodes() != n || m.numTris() != t) throw std::runtime_error("meshops_record: smoothMesh changed the counts");
	REC_CATCH
}

/* killSmallComponents after rebuildQuickCheck() (the plugin reads the corner table without building it); `message` is what it wrote
 * to cout */
int rec_kill(int64_t n, float* pos, float* nrm, int32_t* nflags, int64_t t, int32_t* tris, int32_t* tflags, int elements, int64_t* counts,
             char* message, int64_t message_cap, double* seconds) {
	REC_TRY
	FluidSolver s(Vec3i(8, 8, 8), 3);
	Mesh m(&s);
	fill(m, n, pos, nrm, nflags, t, tris, tflags);
	m.rebuildQuickCheck();
	std::string text;
	{
		CoutCapture cap;
		const double t0 = now();
		killSmallComponents(m, elements);
		if (seconds) *seconds = now() - t0;
		text = cap.text.str();
	}
	if ((int64_t)text.size() + 1 > message_cap) throw std::runtime_error("meshops_record: message buffer too small");
	strcpy(message, text.c_str());
	counts[0] = m.numNodes();
	counts[1] = m.numTris();
	for (int64_t i = 0; i < m.numNodes(); i++) {
		for (int c = 0; c < 3; c++) {
			pos[3 * i + c] = m.nodes(i).pos[c];
			nrm[3 * i + c] = m.nodes(i).normal[c];
		}
		nflags[i] = m.nodes(i).flags;
	}
	for (int64_t i = 0; i < m.numTris(); i++) {
		for (int c = 0; c < 3; c++) tris[3 * i + c] = m.tris(i).c[c];
		tflags[i] = m.tris(i).flags;
	}
	REC_CATCH
}

/* the short pipeline of the GPU test: createMesh on the level set, killSmallComponents (after rebuildQuickCheck), smoothMesh, save;
 * counts = nodes and triangles after createMesh and at the end */
int rec_pipeline(int sx, int sy, int sz, float dt, const float* phi, int elements, float strength, int steps, const char* path, int64_t* counts) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), 3);
	s.mDt = dt;
	LevelsetGrid g(&s);
	for (IndexInt i = 0; i < (IndexInt)sx * sy * sz; i++) g[i] = phi[i];
	Mesh m(&s);
	g.createMesh(m);
	counts[0] = m.numNodes();
	counts[1] = m.numTris();
	m.rebuildQuickCheck();
	{
		CoutCapture cap;
		killSmallComponents(m, elements);
	}
	smoothMesh(m, strength, steps, 1e-5);
	counts[2] = m.numNodes();
	counts[3] = m.numTris();
	m.save(path);
	REC_CATCH
}

}  // extern "C"
