/*
 * tools/surfturb_record.cpp -- the C++ half of the recorder of tests/golden/surfturb.npz (tools/record_surfturb.py is the other half
 * and runs the commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / FlagGrid / BasicParticleSystem
 * objects, calls the reference's own particleSurfaceTurbulence, and -- between whole calls -- the reference's own stage functions
 * one at a time on the state the last call left in its globals.  plugin/surfaceturbulence.cpp is not part of oracle/ref.mk's
 * library: the recorder expands it with the reference's `prep` into oracle/_ref/build/ and this file includes the expanded source,
 * so that the kernels' generated types are visible.  It is linked against oracle/_ref/libmanta_ref.so.  No test runs it; nothing it
 * is compiled with is committed.
 */
#include "plugin/surfaceturbulence.cpp"      // the expanded reference source, from the scratch include path
#include <cstring>
#include <string>

using namespace Manta;
using namespace Manta::SurfaceTurbulence;

namespace {

std::string g_err;
#define REC_TRY try {
#define REC_CATCH                \
	}                            \
	catch (std::exception & e) { \
		g_err = e.what();        \
		return 1;                \
	}                            \
	return 0;

// a BasicParticleSystem whose delete bookkeeping can be read and set
struct Sys : BasicParticleSystem {
	Sys(FluidSolver* s) : BasicParticleSystem(s) {}
	int64_t deletes() const { return mDeletes; }
	int64_t chunk() const { return mDeleteChunk; }
	void book(int64_t d, int64_t c) { mDeletes = d; mDeleteChunk = c; }
};

struct Scene {
	FluidSolver s;
	FlagGrid flags;
	Sys coarse, surf, displaced;
	ParticleDataImpl<Vec3> prev, normals;
	ParticleDataImpl<Real> H, DtH, source, seedAmp, seed;
	Scene(int res)
		: s(Vec3i(res, res, res), 3), flags(&s), coarse(&s), surf(&s), displaced(&s), prev(&s), normals(&s), H(&s), DtH(&s), source(&s), seedAmp(&s), seed(&s) {
		coarse.registerPdata(&prev);
		surf.registerPdata(&normals);
		surf.registerPdata(&H);
		surf.registerPdata(&DtH);
		surf.registerPdata(&source);
		surf.registerPdata(&seedAmp);
		surf.registerPdata(&seed);
	}
};
Scene* g = nullptr;

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

int rec_open(int res, const int32_t* flags) {
	REC_TRY
	delete g;
	g = new Scene(res);
	for (IndexInt i = 0; i < (IndexInt)res * res * res; i++) g->flags[i] = flags[i];
	REC_CATCH
}

// the coarse particles: positions [n][3] and flags; the system is resized (the prev channel with it, old values kept)
int rec_set_coarse(int64_t n, const float* pos, const int32_t* flag) {
	REC_TRY
	g->coarse.resizeAll(n);
	for (int64_t i = 0; i < n; i++) {
		g->coarse[i].pos = Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
		g->coarse[i].flag = flag[i];
	}
	REC_CATCH
}

// the previous positions of the coarse particles, where a loop outside the plugin reorders them (adjustNumber compresses)
int rec_set_prev(const float* prev) {
	REC_TRY
	for (int64_t i = 0; i < g->coarse.size(); i++) g->prev[i] = Vec3(prev[3 * i], prev[3 * i + 1], prev[3 * i + 2]);
	REC_CATCH
}

int rec_call(int res, float outerRadius, int surfaceDensity, int nb, float dt, float waveSpeed, float waveDamping, float waveSeedFrequency,
             float waveMaxAmplitude, float waveMaxFrequency, float waveMaxSeedingAmplitude, float center, float radius, float step) {
	REC_TRY
	particleSurfaceTurbulence(g->flags, g->coarse, g->prev, g->surf, g->normals, g->H, g->DtH, g->displaced, g->source, g->seed, g->seedAmp, res, outerRadius,
	                          surfaceDensity, nb, dt, waveSpeed, waveDamping, waveSeedFrequency, waveMaxAmplitude, waveMaxFrequency, waveMaxSeedingAmplitude,
	                          center, radius, step);
	REC_CATCH
}

// one stage of the reference on the state its globals hold after a call
int rec_stage(const char* name) {
	REC_TRY
	const std::string n(name);
	if (n == "adddelete") addDeleteSurfacePoints(surfacePoints);
	else if (n == "accel") surfacePoints.updateAccel();
	else if (n == "accel_coarse") coarseParticles.updateAccel();
	else if (n == "normals") { computeSurfaceNormals(surfacePoints, coarseParticles, g->normals); smoothSurfaceNormals(surfacePoints, g->normals); }
	else if (n == "regularize") regularizeSurfacePoints(surfacePoints, g->normals);
	else if (n == "constrain") constrainSurface(surfacePoints, coarseParticles);
	else if (n == "waves") surfaceWaves(surfacePoints, g->normals, g->H, g->DtH, g->source, g->seed, g->seedAmp);
	else if (n == "advect") { coarseParticlesPrevPos.updateAccel(); advectSurfacePoints(surfacePoints, coarseParticles, coarseParticlesPrevPos); }
	else throw std::runtime_error("surfturb_record: unknown stage " + n);
	REC_CATCH
}

// sizes[0..5]: surface size, mDeletes, mDeleteChunk, displaced size, frameCount, coarse size
int rec_sizes(int64_t* sizes) {
	sizes[0] = g->surf.size(); sizes[1] = g->surf.deletes(); sizes[2] = g->surf.chunk(); sizes[3] = g->displaced.size(); sizes[4] = frameCount;
	sizes[5] = g->coarse.size();
	return 0;
}
// the surface state: pos[n][3], flag[n], normals[n][3], and the five Real channels [5][n] (H, DtH, source, seed, seedAmp)
int rec_get_surface(float* pos, int32_t* flag, float* normals, float* real) {
	const int64_t n = g->surf.size();
	for (int64_t i = 0; i < n; i++) {
		for (int c = 0; c < 3; c++) { pos[3 * i + c] = g->surf[i].pos[c]; normals[3 * i + c] = g->normals[i][c]; }
		flag[i] = g->surf[i].flag;
		real[i] = g->H[i]; real[n + i] = g->DtH[i]; real[2 * n + i] = g->source[i]; real[3 * n + i] = g->seed[i]; real[4 * n + i] = g->seedAmp[i];
	}
	return 0;
}
int rec_get_coarse(float* pos, int32_t* flag, float* prev) {
	for (int64_t i = 0; i < g->coarse.size(); i++) {
		for (int c = 0; c < 3; c++) { pos[3 * i + c] = g->coarse[i].pos[c]; prev[3 * i + c] = g->prev[i][c]; }
		flag[i] = g->coarse[i].flag;
	}
	return 0;
}
int rec_get_displaced(float* pos) {
	for (int64_t i = 0; i < g->displaced.size(); i++)
		for (int c = 0; c < 3; c++) pos[3 * i + c] = g->displaced[i].pos[c];
	return 0;
}
// the derived parameters as the reference holds them after a call, and the two list resolutions
int rec_get_params(float* out, int32_t* res) {
	const float v[] = {(float)params.res, params.outerRadius, params.innerRadius, params.meanFineDistance, params.constraintA, params.normalRadius,
	                   params.tangentRadius, params.bndXm, params.bndXp};
	memcpy(out, v, sizeof(v));
	res[0] = accelCoarse.res;
	res[1] = accelSurface.res;
	return 0;
}
// cosf(theta) of seedWaves for the frame count the reference holds now: the one host scalar of a call's wave passes
int rec_costheta(float* out) {
	const Real theta = params.dt * frameCount * params.waveSpeed * params.waveSeedFrequency;
	*out = cosf(theta);
	return 0;
}
// the constraint level of every surface slot (the recorder refuses scenes with a level near a threshold)
int rec_levels(float* out) {
	for (int64_t i = 0; i < g->surf.size(); i++) out[i] = computeConstraintLevel(coarseParticles, g->surf[i].pos);
	return 0;
}

}  // extern "C"
