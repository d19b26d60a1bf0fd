/*
 * tools/gridops_record.cpp -- the C++ half of the recorder of tests/golden/gridops.npz (tools/record_gridops.py is the other half; its
 * header has the exact commands).  This file is OUR code: a C ABI that builds the reference's FluidSolver / Grid objects around
 * caller-owned arrays and calls the reference's own Grid::permuteAxes, permuteAxesCopyToGrid, getL1, getL2, join and the plugins
 * addForceField, setForceField, setInitialVelocity, extrapolateVec3Simple, applyEmission, resetInObstacle, copyMACData, copyRealToVec3,
 * copyVec3ToReal, resampleMacToVec3, swapComponents, getGridAvg, debugIntToReal, applySimpleNoiseReal / Vec3, getInterpolated and
 * getNpzFileSize, all of which are in the library of oracle/ref.mk, and the legacy whitewater plugins, whose file is expanded beside it.
 * Linked against oracle/_ref/libmanta_ref.so.  No test runs it; nothing it is compiled with is committed.
 */
#include "manta.h"
#include "grid.h"
#include "levelset.h"
#include "noisefield.h"
#include <cstring>
#include <string>

namespace Manta {
// PYTHON() plugins (plain functions in the NOPYTHON packaging; no header declares them)
void addForceField(const FlagGrid& flags, MACGrid& vel, const Grid<Vec3>& force, const Grid<Real>* region, bool isMAC);
void setForceField(const FlagGrid& flags, MACGrid& vel, const Grid<Vec3>& force, const Grid<Real>* region, bool isMAC);
void setInitialVelocity(const FlagGrid& flags, MACGrid& vel, const Grid<Vec3>& invel);
void extrapolateVec3Simple(Grid<Vec3>& vel, Grid<Real>& phi, int distance, bool inside);
void applyEmission(FlagGrid& flags, Grid<Real>& target, Grid<Real>& source, Grid<Real>* emissionTexture, bool isAbsolute, int type);
void resetInObstacle(FlagGrid& flags, MACGrid& vel, Grid<Real>* density, Grid<Real>* heat, Grid<Real>* fuel, Grid<Real>* flame, Grid<Real>* red,
                     Grid<Real>* green, Grid<Real>* blue, Real resetValue);
void copyMACData(const MACGrid& source, MACGrid& target, const FlagGrid& flags, const int flag, const int bnd);
void copyRealToVec3(Grid<Real>& sourceX, Grid<Real>& sourceY, Grid<Real>& sourceZ, Grid<Vec3>& target);
void copyVec3ToReal(Grid<Vec3>& source, Grid<Real>& targetX, Grid<Real>& targetY, Grid<Real>& targetZ);
void resampleMacToVec3(MACGrid& source, Grid<Vec3>& target);
void swapComponents(Grid<Vec3>& vel, int c1, int c2, int c3);
Real getGridAvg(Grid<Real>& source, FlagGrid* flags);
void debugIntToReal(const Grid<int>& source, Grid<Real>& dest, Real factor);
Vec3 getNpzFileSize(const std::string& name);
void applySimpleNoiseVec3(const FlagGrid& flags, Grid<Vec3>& target, const WaveletNoiseField& noise, Real scale, const Grid<Real>* weight);
void applySimpleNoiseReal(const FlagGrid& flags, Grid<Real>& target, const WaveletNoiseField& noise, Real scale, const Grid<Real>* weight);
// plugin/secondaryparticles.cpp is not in the library of oracle/ref.mk: the recorder is linked with its expansion (record_gridops.py)
void flipComputePotentialTrappedAir(Grid<Real>& pot, const FlagGrid& flags, const MACGrid& v, const int radius, const Real tauMin, const Real tauMax,
                                    const Real scaleFromManta, const int itype, const int jtype);
void flipComputePotentialKineticEnergy(Grid<Real>& pot, const FlagGrid& flags, const MACGrid& v, const Real tauMin, const Real tauMax,
                                       const Real scaleFromManta, const int itype);
void flipComputePotentialWaveCrest(Grid<Real>& pot, const FlagGrid& flags, const MACGrid& v, const int radius, Grid<Vec3>& normal, const Real tauMin,
                                   const Real tauMax, const Real scaleFromManta, const int itype, const int jtype);
void flipComputeSurfaceNormals(Grid<Vec3>& normal, const Grid<Real>& phi);
void flipUpdateNeighborRatio(const FlagGrid& flags, Grid<Real>& neighborRatio, const int radius, const int itype, const int jtype);
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

template <class G>
IndexInt cells(const G& g) {
	return g.getSizeX() * (IndexInt)g.getSizeY() * g.getSizeZ();
}
// Real and int grids cross as they are; Vec3 grids cross element-major: [n][3]
void load(Grid<Real>& g, const void* a) {
	for (IndexInt i = 0; i < cells(g); i++) g[i] = ((const float*)a)[i];
}
void load(Grid<int>& g, const void* a) {
	for (IndexInt i = 0; i < cells(g); i++) g[i] = ((const int32_t*)a)[i];
}
void load(Grid<Vec3>& g, const void* a) {
	const float* f = (const float*)a;
	for (IndexInt i = 0; i < cells(g); i++) g[i] = Vec3(f[3 * i], f[3 * i + 1], f[3 * i + 2]);
}
void store(const Grid<Real>& g, void* a) {
	for (IndexInt i = 0; i < cells(g); i++) ((float*)a)[i] = g[i];
}
void store(const Grid<int>& g, void* a) {
	for (IndexInt i = 0; i < cells(g); i++) ((int32_t*)a)[i] = g[i];
}
void store(const Grid<Vec3>& g, void* a) {
	float* f = (float*)a;
	for (IndexInt i = 0; i < cells(g); i++)
		for (int c = 0; c < 3; c++) f[3 * i + c] = g[i][c];
}
int dim_of(int sz) { return sz > 1 ? 3 : 2; }

template <class G>
void permute(int sx, int sy, int sz, int a0, int a1, int a2, int tx, int ty, int tz, int inplace, const void* in, void* out) {
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	G g(&s);
	load(g, in);
	if (inplace) {
		g.permuteAxes(a0, a1, a2);
		store(g, out);
	} else {
		FluidSolver t(Vec3i(tx, ty, tz), dim_of(tz));
		G o(&t);
		load(o, out);
		g.permuteAxesCopyToGrid(a0, a1, a2, o);
		store(o, out);
	}
}
template <class G>
float norm_of(int l2, int sx, int sy, int sz, int bnd, const void* a) {
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	G g(&s);
	load(g, a);
	return l2 ? g.getL2(bnd) : g.getL1(bnd);
}
template <class G>
void join_of(int sx, int sy, int sz, void* a, const void* b, int keepMax) {
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	G g(&s), o(&s);
	load(g, a);
	load(o, b);
	g.join(o, keepMax != 0);
	store(g, a);
}

}  // namespace

extern "C" {

const char* rec_last_error(void) { return g_err.c_str(); }

/* kind 0 Grid<Real>, 1 Grid<int>, 2 Grid<Vec3>.  inplace: permuteAxes, the result in out; else permuteAxesCopyToGrid into a grid of the
 * solver (tx, ty, tz) that starts as out */
int rec_permute(int kind, int sx, int sy, int sz, int a0, int a1, int a2, int tx, int ty, int tz, int inplace, const void* in, void* out) {
	REC_TRY
	if (kind == 0) permute<Grid<Real> >(sx, sy, sz, a0, a1, a2, tx, ty, tz, inplace, in, out);
	else if (kind == 1) permute<Grid<int> >(sx, sy, sz, a0, a1, a2, tx, ty, tz, inplace, in, out);
	else permute<Grid<Vec3> >(sx, sy, sz, a0, a1, a2, tx, ty, tz, inplace, in, out);
	REC_CATCH
}

int rec_norm(int kind, int l2, int sx, int sy, int sz, int bnd, const void* a, float* out) {
	REC_TRY
	*out = kind == 0 ? norm_of<Grid<Real> >(l2, sx, sy, sz, bnd, a) : kind == 1 ? norm_of<Grid<int> >(l2, sx, sy, sz, bnd, a)
	                                                                          : norm_of<Grid<Vec3> >(l2, sx, sy, sz, bnd, a);
	REC_CATCH
}

int rec_join(int kind, int sx, int sy, int sz, void* a, const void* b, int keepMax) {
	REC_TRY
	if (kind == 0) join_of<Grid<Real> >(sx, sy, sz, a, b, keepMax);
	else if (kind == 1) join_of<Grid<int> >(sx, sy, sz, a, b, keepMax);
	else join_of<Grid<Vec3> >(sx, sy, sz, a, b, keepMax);
	REC_CATCH
}

int rec_force_field(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* force, const float* region, int additive, int isMAC) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	FlagGrid f(&s);
	MACGrid v(&s);
	Grid<Vec3> fo(&s);
	Grid<Real> r(&s);
	load(f, flags); load(v, vel); load(fo, force);
	if (region) load(r, region);
	if (additive) addForceField(f, v, fo, region ? &r : NULL, isMAC != 0);
	else setForceField(f, v, fo, region ? &r : NULL, isMAC != 0);
	store(v, vel);
	REC_CATCH
}

int rec_initial_velocity(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* invel) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	FlagGrid f(&s);
	MACGrid v(&s);
	Grid<Vec3> fo(&s);
	load(f, flags); load(v, vel); load(fo, invel);
	setInitialVelocity(f, v, fo);
	store(v, vel);
	REC_CATCH
}

int rec_extrapolate_vec3(int sx, int sy, int sz, float* vel, const float* phi, int distance, int inside) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	Grid<Vec3> v(&s);
	Grid<Real> p(&s);
	load(v, vel); load(p, phi);
	extrapolateVec3Simple(v, p, distance, inside != 0);
	store(v, vel);
	REC_CATCH
}

int rec_emission(int sx, int sy, int sz, const int32_t* flags, float* target, const float* source, const float* tex, int isAbsolute, int type) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	FlagGrid f(&s);
	Grid<Real> t(&s), so(&s), te(&s);
	load(f, flags); load(t, target); load(so, source);
	if (tex) load(te, tex);
	applyEmission(f, t, so, tex ? &te : NULL, isAbsolute != 0, type);
	store(t, target);
	REC_CATCH
}

/* g: seven pointers (density, heat, fuel, flame, red, green, blue), NULL where the grid is not given; written back in place */
int rec_reset_in_obstacle(int sx, int sy, int sz, const int32_t* flags, float* vel, float** g, float value) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	FlagGrid f(&s);
	MACGrid v(&s);
	Grid<Real> a0(&s), a1(&s), a2(&s), a3(&s), a4(&s), a5(&s), a6(&s);
	Grid<Real>* G[7] = {&a0, &a1, &a2, &a3, &a4, &a5, &a6};
	load(f, flags); load(v, vel);
	for (int q = 0; q < 7; q++)
		if (g[q]) load(*G[q], g[q]);
		else G[q] = NULL;
	resetInObstacle(f, v, G[0], G[1], G[2], G[3], G[4], G[5], G[6], value);
	store(v, vel);
	for (int q = 0; q < 7; q++)
		if (g[q]) store(*G[q], g[q]);
	REC_CATCH
}

int rec_copy_mac_data(int sx, int sy, int sz, const float* source, float* target, const int32_t* flags, int flag, int bnd) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	FlagGrid f(&s);
	MACGrid so(&s), t(&s);
	load(f, flags); load(so, source); load(t, target);
	copyMACData(so, t, f, flag, bnd);
	store(t, target);
	REC_CATCH
}

int rec_real_to_vec3(int sx, int sy, int sz, const float* x, const float* y, const float* z, float* target) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	Grid<Real> gx(&s), gy(&s), gz(&s);
	Grid<Vec3> t(&s);
	load(gx, x); load(gy, y); load(gz, z); load(t, target);
	copyRealToVec3(gx, gy, gz, t);
	store(t, target);
	REC_CATCH
}

int rec_vec3_to_real(int sx, int sy, int sz, const float* source, float* x, float* y, float* z) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	Grid<Real> gx(&s), gy(&s), gz(&s);
	Grid<Vec3> so(&s);
	load(gx, x); load(gy, y); load(gz, z); load(so, source);
	copyVec3ToReal(so, gx, gy, gz);
	store(gx, x); store(gy, y); store(gz, z);
	REC_CATCH
}

int rec_resample_mac_to_vec3(int sx, int sy, int sz, const float* source, float* target) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	MACGrid so(&s);
	Grid<Vec3> t(&s);
	load(so, source); load(t, target);
	resampleMacToVec3(so, t);
	store(t, target);
	REC_CATCH
}

int rec_swap_components(int sx, int sy, int sz, float* vel, int c1, int c2, int c3) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	Grid<Vec3> v(&s);
	load(v, vel);
	swapComponents(v, c1, c2, c3);
	store(v, vel);
	REC_CATCH
}

int rec_grid_avg(int sx, int sy, int sz, const float* source, const int32_t* flags, float* out) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	Grid<Real> so(&s);
	FlagGrid f(&s);
	load(so, source);
	if (flags) load(f, flags);
	*out = getGridAvg(so, flags ? &f : NULL);
	REC_CATCH
}

/* set 0: a default field; set 1: posScale (2.5, 1.5, 0.75), valOffset 0.1, clamp to [-0.2, 0.3].  fixedSeed -1, no tile file */
int rec_simple_noise(int vec, int sx, int sy, int sz, const int32_t* flags, float* target, const float* weight, float scale, int set) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	WaveletNoiseField noise(&s, -1, 0);
	if (set == 1) {
		noise.mPosScale = Vec3(2.5, 1.5, 0.75);
		noise.mValOffset = 0.1;
		noise.mClamp = true;
		noise.mClampNeg = -0.2;
		noise.mClampPos = 0.3;
	}
	FlagGrid f(&s);
	Grid<Real> w(&s);
	load(f, flags);
	if (weight) load(w, weight);
	if (vec) {
		Grid<Vec3> t(&s);
		load(t, target);
		applySimpleNoiseVec3(f, t, noise, scale, weight ? &w : NULL);
		store(t, target);
	} else {
		Grid<Real> t(&s);
		load(t, target);
		applySimpleNoiseReal(f, t, noise, scale, weight ? &w : NULL);
		store(t, target);
	}
	REC_CATCH
}

/* which 0 trapped air, 1 wave crest, 2 kinetic energy, 3 neighbour ratio (pot is the ratio grid), 4 surface normals (normal in place) */
int rec_legacy(int which, int sx, int sy, int sz, float* pot, const int32_t* flags, const float* vel, float* normal, const float* phi,
               int radius, float tauMin, float tauMax, float scale, int itype, int jtype) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	Grid<Real> p(&s), ph(&s);
	FlagGrid f(&s);
	MACGrid v(&s);
	Grid<Vec3> nrm(&s);
	if (pot) load(p, pot);
	if (flags) load(f, flags);
	if (vel) load(v, vel);
	if (normal) load(nrm, normal);
	if (phi) load(ph, phi);
	if (which == 0) flipComputePotentialTrappedAir(p, f, v, radius, tauMin, tauMax, scale, itype, jtype);
	else if (which == 1) flipComputePotentialWaveCrest(p, f, v, radius, nrm, tauMin, tauMax, scale, itype, jtype);
	else if (which == 2) flipComputePotentialKineticEnergy(p, f, v, tauMin, tauMax, scale, itype);
	else if (which == 3) flipUpdateNeighborRatio(f, p, radius, itype, jtype);
	else flipComputeSurfaceNormals(nrm, ph);
	if (pot) store(p, pot);
	if (which == 4) store(nrm, normal);
	REC_CATCH
}

/* kind 0 Grid<Real>, 2 Grid<Vec3>, 3 MACGrid: getInterpolated at np positions [np][3] -> out [np][3] (a Real grid fills out[q][0]) */
int rec_interpolated(int kind, int sx, int sy, int sz, const float* data, int np, const float* pos, float* out) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	Grid<Real> r(&s);
	Grid<Vec3> v(&s);
	MACGrid m(&s);
	if (kind == 0) load(r, data);
	else if (kind == 2) load(v, data);
	else load(m, data);
	for (int q = 0; q < np; q++) {
		const Vec3 p(pos[3 * q], pos[3 * q + 1], pos[3 * q + 2]);
		Vec3 o(0.);
		if (kind == 0) o.x = r.getInterpolated(p);
		else if (kind == 2) o = v.getInterpolated(p);
		else o = m.getInterpolated(p);
		for (int c = 0; c < 3; c++) out[3 * q + c] = o[c];
	}
	REC_CATCH
}

int rec_npz_file_size(const char* name, float* out) {
	REC_TRY
	const Vec3 v = getNpzFileSize(std::string(name));
	for (int c = 0; c < 3; c++) out[c] = v[c];
	REC_CATCH
}

int rec_int_to_real(int sx, int sy, int sz, const int32_t* source, float* dest, float factor) {
	REC_TRY
	FluidSolver s(Vec3i(sx, sy, sz), dim_of(sz));
	Grid<int> so(&s);
	Grid<Real> d(&s);
	load(so, source); load(d, dest);
	debugIntToReal(so, d, factor);
	store(d, dest);
	REC_CATCH
}

}  // extern "C"
