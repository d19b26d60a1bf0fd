// surfturb_cells.h -- the per-point bodies of surfturb.hip (surface turbulence, plugin/surfaceturbulence.cpp) as __host__ __device__
// functions: the kernels call them with one thread per point, and a stand-alone host program (tools/surfturb_host_check.hip) calls the
// same text in serial loops, where the host sanitizers can watch every index.  Contract, quirks and fp32 / fp64 map: DESIGN.md section 27.
// Built with -ffp-contract=off.  Everything is fp32 in the reference's evaluation order unless a comment says otherwise.
#pragma once
#include "common.h"
#include <limits.h>
#include <math.h>

namespace mf {
namespace surfturb {

#define ST_HD __host__ __device__ __forceinline__

constexpr int PNEW = 1, PDELETE = 1 << 10;    // ParticleBase::PNEW / PDELETE, particle.h
constexpr int NPAR = 32;

// the parameter block, NPAR floats written by mf_surfturb_params (host) and handed to every device entry
struct Par {
	float res;              // (float)params.res
	float outerRadius, innerRadius, meanFineDistance, constraintA, normalRadius, tangentRadius, bndm, bndp;
	float dt, waveSpeed, waveDamping, waveSeedFrequency, waveMaxAmplitude, waveMaxFrequency, waveMaxSeedingAmplitude;
	float curvCenter, curvRadius, seedStep;
	float costheta;         // cosf(dt * frameCount * waveSpeed * waveSeedFrequency), one host scalar per call
	float addRadius;        // Real(meanFineDistance - 1e-6), the double difference rounded once
	float delRadius;        // Real(0.67 * meanFineDistance)
	float dtheta;           // 2 * meanFineDistance / (outerRadius + innerRadius)
	float pad[NPAR - 23];
};
static_assert(sizeof(Par) == NPAR * sizeof(float), "Par is NPAR floats");

struct V3 {
	float x, y, z;
};
ST_HD V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
ST_HD V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
ST_HD V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
ST_HD V3 operator*(float s, V3 v) { return {v.x * s, v.y * s, v.z * s}; }
ST_HD V3 operator*(V3 v, float s) { return {v.x * s, v.y * s, v.z * s}; }
ST_HD V3 operator/(V3 v, float s) { return {v.x / s, v.y / s, v.z / s}; }
ST_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
ST_HD V3 cross(V3 t, V3 v) { return {(t.y * v.z) - (t.z * v.y), (t.z * v.x) - (t.x * v.z), (t.x * v.y) - (t.y * v.x)}; }
ST_HD float norm_square(V3 v) { return v.x * v.x + v.y * v.y + v.z * v.z; }
// norm / getNormalized, vectorbase.h:384-416, S = float: |v|^2 in float, the "== 1" test in double, fac = (float)(1. / sqrt((double)l))
ST_HD float norm(V3 v) {
	const float l = v.x * v.x + v.y * v.y + v.z * v.z;
	const float eps2 = 1e-6f * 1e-6f;
	if (l <= eps2) return 0.f;
	return (fabs((double)l - 1.) < (double)eps2) ? 1.f : sqrtf(l);
}
ST_HD V3 normalized(V3 v) {
	const float l = v.x * v.x + v.y * v.y + v.z * v.z;
	const float eps2 = 1e-6f * 1e-6f;
	if (fabs((double)l - 1.) < (double)eps2) return v;
	if (l > eps2) {
		const float fac = (float)(1. / sqrt((double)l));
		return {v.x * fac, v.y * fac, v.z * fac};
	}
	return {0.f, 0.f, 0.f};
}
// expf / logf of the reference: here the fp64 function of the widened argument, rounded once (the only transcendentals on the device)
ST_HD float st_expf(float x) { return (float)exp((double)x); }
ST_HD float st_logf(float x) { return (float)log((double)x); }
ST_HD float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }     // general.h:137: a NaN passes through

// a point set pos[3][cap], flag[cap] of n slots; flag == nullptr: every slot is active (the list over coarsePartsPrevPos)
struct Pts {
	int64_t n, cap;
	const float* pos;
	const int32_t* flag;
};
ST_HD V3 pos_of(const Pts& P, int64_t i) { return {P.pos[i], P.pos[P.cap + i], P.pos[2 * P.cap + i]}; }
ST_HD bool active(const Pts& P, int64_t i) { return !P.flag || (P.flag[i] & PDELETE) == 0; }

// a cell list of R^3 cells: the slots of cell c are ids[start[c] .. start[c + 1]), ascending
struct Cells {
	int R;
	const int32_t* start;
	const int32_t* ids;
};
// float -> int as x86-64 converts (cvttss2si): NaN and everything outside int's range give INT_MIN
ST_HD int cvt_x86(float f) { return (f >= -2147483648.f && f < 2147483648.f) ? (int)f : INT_MIN; }
// clamp<int>(floor(v / params.res * R), 0, R - 1)
ST_HD int cell_coord(float v, float res, int R) {
	const int c = cvt_x86(floorf(v / res * (float)R));
	return c < 0 ? 0 : (c > R - 1 ? R - 1 : c);
}
ST_HD int64_t cell_of(V3 p, float res, int R) {
	return ((int64_t)cell_coord(p.x, res, R) * R + cell_coord(p.y, res, R)) * R + cell_coord(p.z, res, R);
}

// LOOP_NEIGHBORS_BEGIN / END, surfaceturbulence.cpp:128-144: cells i outer, j, k inner, slots ascending, inactive slots skipped at query
// time.  `idn` is the neighbour; `break` leaves the slot loop of one cell only, as in the reference
#define ST_NEIGHBOURS_BEGIN(par, C, P, center, radius)                                                                      \
	{                                                                                                                       \
		const int lo0_ = cell_coord((center).x - (radius), (par).res, (C).R), hi0_ = cell_coord((center).x + (radius), (par).res, (C).R); \
		const int lo1_ = cell_coord((center).y - (radius), (par).res, (C).R), hi1_ = cell_coord((center).y + (radius), (par).res, (C).R); \
		const int lo2_ = cell_coord((center).z - (radius), (par).res, (C).R), hi2_ = cell_coord((center).z + (radius), (par).res, (C).R); \
		for (int ci_ = lo0_; ci_ <= hi0_; ci_++)                                                                            \
			for (int cj_ = lo1_; cj_ <= hi1_; cj_++)                                                                        \
				for (int ck_ = lo2_; ck_ <= hi2_; ck_++) {                                                                  \
					const int64_t cell_ = ((int64_t)ci_ * (C).R + cj_) * (C).R + ck_;                                       \
					const int32_t end_ = (C).start[cell_ + 1];                                                              \
					for (int32_t s_ = (C).start[cell_]; s_ < end_; s_++) {                                                  \
						const int32_t idn = (C).ids[s_];                                                                    \
						if (active(P, idn)) {
#define ST_NEIGHBOURS_END \
	}                     \
	}                     \
	}                     \
	}

// LOOP_GHOSTS_*, :146-169: the next entry of the chain after `flag` for the NEIGHBOUR p: its mirror images at the planes it is within
// radius of, x-, x+, y-, y+, z-, z+ in this order, then (flag 6) the neighbour itself.  g is the image; the image's normal has the
// component flag / 2 negated (flag < 6)
ST_HD int ghost_next(const Par& par, int flag, V3 p, float radius, V3& g) {
	if (flag < 0 && p.x - par.bndm <= radius) { g = {2.f * par.bndm - p.x, p.y, p.z}; return 0; }
	if (flag < 1 && par.bndp - p.x <= radius) { g = {2.f * par.bndp - p.x, p.y, p.z}; return 1; }
	if (flag < 2 && p.y - par.bndm <= radius) { g = {p.x, 2.f * par.bndm - p.y, p.z}; return 2; }
	if (flag < 3 && par.bndp - p.y <= radius) { g = {p.x, 2.f * par.bndp - p.y, p.z}; return 3; }
	if (flag < 4 && p.z - par.bndm <= radius) { g = {p.x, p.y, 2.f * par.bndm - p.z}; return 4; }
	if (flag < 5 && par.bndp - p.z <= radius) { g = {p.x, p.y, 2.f * par.bndp - p.z}; return 5; }
	g = p;
	return 6;
}
ST_HD V3 ghost_normal(int flag, V3 n) {
	if (flag == 0 || flag == 1) return {-n.x, n.y, n.z};
	if (flag == 2 || flag == 3) return {n.x, -n.y, n.z};
	if (flag == 4 || flag == 5) return {n.x, n.y, -n.z};
	return n;
}

ST_HD float triangular(float distance, float radius) { return 1.0f - distance / radius; }
ST_HD float weight_radius(float distance, float radius) { return distance > radius ? 0.f : triangular(distance, radius); }
ST_HD bool in_domain(const Par& par, V3 p) {
	return par.bndm <= p.x && p.x <= par.bndp && par.bndm <= p.y && p.y <= par.bndp && par.bndm <= p.z && p.z <= par.bndp;
}

// computeConstraintLevel / computeConstraintGradient, :438-460
ST_HD float constraint_level(const Par& par, const Cells& CC, const Pts& coarse, V3 pos) {
	float lvl = 0.0f;
	const float r = 1.5f * par.outerRadius;
	ST_NEIGHBOURS_BEGIN(par, CC, coarse, pos, r)
	lvl += st_expf(-par.constraintA * norm_square(pos_of(coarse, idn) - pos));
	ST_NEIGHBOURS_END
	if (lvl > 1.0f) lvl = 1.0f;
	return (sqrtf(-st_logf(lvl) / par.constraintA) - par.innerRadius) / (par.outerRadius - par.innerRadius);
}
ST_HD V3 constraint_gradient(const Par& par, const Cells& CC, const Pts& coarse, V3 pos) {
	V3 g = {0.f, 0.f, 0.f};
	const float r = 1.5f * par.outerRadius;
	ST_NEIGHBOURS_BEGIN(par, CC, coarse, pos, r)
	const V3 cp = pos_of(coarse, idn);
	g = g + (2.f * par.constraintA * st_expf(-par.constraintA * norm_square(cp - pos))) * (pos - cp);
	ST_NEIGHBOURS_END
	return normalized(g);
}
// hasNeighbor, :200-220
ST_HD bool has_neighbour(const Par& par, const Cells& C, const Pts& P, V3 pos, float radius) {
	bool answer = false;
	ST_NEIGHBOURS_BEGIN(par, C, P, pos, radius)
	if (norm(pos_of(P, idn) - pos) <= radius) answer = true;
	ST_NEIGHBOURS_END
	return answer;
}

// initFines, :349-401, for coarse particle p and direction d of the host's table: 1 and the position if a surface point is created
ST_HD int init_fine(const Par& par, const Cells& CC, const Pts& coarse, int sx, int sy, int sz, const int32_t* gridflags, int64_t p, V3 dir, V3& out) {
	if (!active(coarse, p)) return 0;
	const V3 pos = pos_of(coarse, p);
	bool near = false;
	for (int i = -1; i <= 1; i++)
		for (int j = -1; j <= 1; j++)
			for (int k = -1; k <= 1; k++) {
				// the precondition keeps these inside the grid (coarse particles sit in cells [1, size - 2]); the clamp is for memory safety only
				int x = (int)pos.x + i, y = (int)pos.y + j, z = (int)pos.z + k;
				x = x < 0 ? 0 : (x > sx - 1 ? sx - 1 : x);
				y = y < 0 ? 0 : (y > sy - 1 ? sy - 1 : y);
				z = z < 0 ? 0 : (z > sz - 1 ? sz - 1 : z);
				if (!(gridflags[((int64_t)z * sy + y) * sx + x] & 1)) near = true;     // FlagGrid::TypeFluid
			}
	if (!near) return 0;
	out = pos + par.outerRadius * dir;
	const float r = 2.f * par.outerRadius, r2 = par.outerRadius * par.outerRadius;
	bool valid = true;
	ST_NEIGHBOURS_BEGIN(par, CC, coarse, out, r)
	if (p != idn && norm_square(out - pos_of(coarse, idn)) < r2) valid = false;
	ST_NEIGHBOURS_END
	return valid ? 1 : 0;
}

// advectSurfacePoints, :407-432; CP is the list over prev (every slot active), coarse carries the flags
ST_HD V3 advect_point(const Par& par, const Cells& CP, const Pts& prev, const Pts& coarse, V3 p) {
	V3 avg = {0.f, 0.f, 0.f};
	float total = 0.f;
	const float r = 2.0f * par.outerRadius;
	ST_NEIGHBOURS_BEGIN(par, CP, prev, p, r)
	if ((coarse.flag[idn] & PNEW) == 0 && (coarse.flag[idn] & PDELETE) == 0) {
		const V3 pp = pos_of(prev, idn);
		const V3 disp = pos_of(coarse, idn) - pp;
		const float w = weight_radius(norm(pp - p), r);
		avg = avg + w * disp;
		total += w;
	}
	ST_NEIGHBOURS_END
	if (total != 0.f) avg = avg / total;
	return p + avg;
}

// the add pass of addDeleteSurfacePoints, :566-602, for slot idx (deleted slots included): 1 and the position of the buffered point
ST_HD int add_candidate(const Par& par, const Cells& CC, const Pts& coarse, const Cells& CS, const Pts& surf, int64_t idx, V3& out) {
	const V3 pos = pos_of(surf, idx);
	const V3 gradient = constraint_gradient(par, CC, coarse, pos);
	float wt = 0.f;
	V3 td = {0.f, 0.f, 0.f};
	ST_NEIGHBOURS_BEGIN(par, CS, surf, pos, par.tangentRadius)
	if (idn != idx) {
		V3 dir = pos - pos_of(surf, idn);
		const float length = norm(dir);
		dir = normalized(dir);
		const V3 dn = dot(dir, gradient) * gradient;
		const V3 dt = dir - dn;
		const float w = weight_radius(length, par.tangentRadius);
		wt += w;
		td = td + w * dt;
	}
	ST_NEIGHBOURS_END
	(void)wt;
	if (norm(td) != 0.f) td = normalized(td);
	out = pos + par.meanFineDistance * td;
	return (in_domain(par, out) && !has_neighbour(par, CS, surf, out, par.addRadius)) ? 1 : 0;
}

// delete pass 1, :611-618, stated in rounds: slot i is decided once its lower listed neighbours within range are.  state: 0 undecided,
// 1 kept, 2 killed.  A slot outside the domain is killed at once; higher listed neighbours count as still active, lower ones with their
// decision; neighbours deleted before the pass are skipped by the query.  Returns the new state of i
ST_HD int greedy_decide(const Par& par, const Cells& CS, const Pts& surf, const int32_t* state, int64_t i) {
	const V3 pos = pos_of(surf, i);
	if (!in_domain(par, pos)) return 2;
	bool hit = false, wait = false;
	ST_NEIGHBOURS_BEGIN(par, CS, surf, pos, par.delRadius)
	if (idn != i && norm(pos_of(surf, idn) - pos) <= par.delRadius) {
		if (idn > i)
			hit = true;
		else if (state[idn] == 0)
			wait = true;
		else if (state[idn] == 1)
			hit = true;
	}
	ST_NEIGHBOURS_END
	return wait ? 0 : (hit ? 2 : 1);
}
// passes 2 and 3, :621-636: bit 0 no coarse neighbour within 2 outerRadius, bit 1 level outside [-0.2, 1.2] (compared in double)
ST_HD int delete_coarse(const Par& par, const Cells& CC, const Pts& coarse, V3 pos) {
	int r = has_neighbour(par, CC, coarse, pos, 2.f * par.outerRadius) ? 0 : 1;
	const float level = constraint_level(par, CC, coarse, pos);
	if ((double)level < -0.2 || (double)level > 1.2) r |= 2;
	return r;
}

// the tangent frame of computeSurfaceNormals / computeSurfaceWaveNormal / computeSurfaceWaveLaplacians
ST_HD void tangent_frame(V3 n, V3& t1, V3& t2) {
	const V3 vx = {1.f, 0.f, 0.f}, vy = {0.f, 1.f, 0.f};
	const float dotX = dot(n, vx), dotY = dot(n, vy);
	t1 = normalized(fabsf(dotX) < fabsf(dotY) ? cross(n, vx) : cross(n, vy));
	t2 = normalized(cross(n, t1));
}
struct Fit {
	float sw, swx, swy, swxy, swx2, swy2, swxz, swyz, swz;
};
ST_HD void fit_add(Fit& f, float w, float x, float y, float z) {
	f.swx2 += w * x * x;
	f.swy2 += w * y * y;
	f.swxy += w * x * y;
	f.swxz += w * x * z;
	f.swyz += w * y * z;
	f.swx += w * x;
	f.swy += w * y;
	f.swz += w * z;
	f.sw += w;
}
ST_HD float fit_det(const Fit& f) {
	return -f.sw * f.swxy * f.swxy + 2.f * f.swx * f.swxy * f.swy - f.swx2 * f.swy * f.swy - f.swx * f.swx * f.swy2 + f.sw * f.swx2 * f.swy2;
}
ST_HD V3 fit_abc(const Fit& f, float det) {
	const V3 v = {f.swxz * (-f.swy * f.swy + f.sw * f.swy2) + f.swyz * (-f.sw * f.swxy + f.swx * f.swy) + f.swz * (f.swxy * f.swy - f.swx * f.swy2),
	              f.swxz * (-f.sw * f.swxy + f.swx * f.swy) + f.swyz * (-f.swx * f.swx + f.sw * f.swx2) + f.swz * (f.swx * f.swxy - f.swx2 * f.swy),
	              f.swxz * (f.swxy * f.swy - f.swx * f.swy2) + f.swyz * (f.swx * f.swxy - f.swx2 * f.swy) + f.swz * (-f.swxy * f.swxy + f.swx2 * f.swy2)};
	return (1.f / det) * v;
}

// computeSurfaceNormals, :467-518
ST_HD V3 surface_normal(const Par& par, const Cells& CC, const Pts& coarse, const Cells& CS, const Pts& surf, int64_t idx) {
	const V3 pos = pos_of(surf, idx);
	const V3 gradient = constraint_gradient(par, CC, coarse, pos);
	const V3 n = normalized(gradient);
	V3 t1, t2;
	tangent_frame(n, t1, t2);
	Fit f = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
	ST_NEIGHBOURS_BEGIN(par, CS, surf, pos, par.normalRadius)
	const V3 q = pos_of(surf, idn);
	int gf = -1;
	V3 g;
	while (gf < 6) {
		gf = ghost_next(par, gf, q, par.normalRadius, g);
		const float x = dot(g - pos, t1), y = dot(g - pos, t2), z = dot(g - pos, n);
		fit_add(f, weight_radius(norm(pos - g), par.normalRadius), x, y, z);
	}
	ST_NEIGHBOURS_END
	const float det = fit_det(f);
	if (det == 0.f) return {0.f, 0.f, 0.f};
	const V3 abc = fit_abc(f, det);
	V3 normal = -normalized(t1 * abc.x + t2 * abc.y - n);
	if (dot(gradient, normal) < 0.f) normal = -normal;
	return normal;
}
// computeAveragedNormals, :525-537; normals[3][cap]
ST_HD V3 vec_of(const float* a, int64_t cap, int64_t i) { return {a[i], a[cap + i], a[2 * cap + i]}; }
ST_HD V3 averaged_normal(const Par& par, const Cells& CS, const Pts& surf, const float* normals, int64_t idx) {
	const V3 pos = pos_of(surf, idx);
	V3 nn = {0.f, 0.f, 0.f};
	ST_NEIGHBOURS_BEGIN(par, CS, surf, pos, par.normalRadius)
	const float w = weight_radius(norm(pos - pos_of(surf, idn)), par.normalRadius);
	nn = nn + w * vec_of(normals, surf.cap, idn);
	ST_NEIGHBOURS_END
	return normalized(nn);
}

// computeSurfaceDensities, :648-661
ST_HD float surface_density(const Par& par, const Cells& CS, const Pts& surf, int64_t idx) {
	const V3 pos = pos_of(surf, idx);
	float density = 0.f;
	ST_NEIGHBOURS_BEGIN(par, CS, surf, pos, par.normalRadius)
	const V3 q = pos_of(surf, idn);
	int gf = -1;
	V3 g;
	while (gf < 6) {
		gf = ghost_next(par, gf, q, par.normalRadius, g);
		density += weight_radius(norm(pos - g), par.normalRadius);
	}
	ST_NEIGHBOURS_END
	return density;
}
// computeSurfaceDisplacements, :663-702; density[n]
ST_HD V3 surface_displacement(const Par& par, const Cells& CS, const Pts& surf, const float* normals, const float* density, int64_t idx) {
	const V3 pos = pos_of(surf, idx);
	const V3 normal = vec_of(normals, surf.cap, idx);
	V3 dN = {0.f, 0.f, 0.f}, dT = {0.f, 0.f, 0.f};
	float wTotal = 0.f;
	ST_NEIGHBOURS_BEGIN(par, CS, surf, pos, par.normalRadius)
	const V3 q = pos_of(surf, idn), qn = vec_of(normals, surf.cap, idn);
	int gf = -1;
	V3 g;
	while (gf < 6) {
		gf = ghost_next(par, gf, q, par.normalRadius, g);
		const V3 gNormal = ghost_normal(gf, qn);
		const V3 dir = pos - g;
		const float length = norm(dir);
		V3 dn = dot(dir, normal) * normal;
		const V3 dt = dir - dn;
		if (density[idn] == 0.f) continue;
		const float w = weight_radius(length, par.normalRadius) / density[idn];
		const V3 crossVec = normalized(cross(normal, -dir));
		const V3 projected = normalized(gNormal - dot(crossVec, gNormal) * crossVec);
		if (dot(projected, normal) < 0.f || (double)fabsf(dot(normal, normal + projected)) < 1e-6) continue;
		dn = (-dot(normal + projected, dir) / dot(normal, normal + projected)) * normal;
		dN = dN + w * dn;
		dT = dT + w * normalized(dt);
		wTotal += w;
	}
	ST_NEIGHBOURS_END
	if (wTotal != 0.f) {
		dN = dN / wTotal;
		dT = dT / wTotal;
	}
	dN = dN * .75f;
	dT = dT * (.25f * par.meanFineDistance);
	return dN + dT;
}
// constrainSurface, :726-738
ST_HD V3 constrained(const Par& par, const Cells& CC, const Pts& coarse, V3 pos) {
	const float level = constraint_level(par, CC, coarse, pos);
	if (level > 1.f) return pos - ((par.outerRadius - par.innerRadius) * (level - 1.f)) * constraint_gradient(par, CC, coarse, pos);
	if (level < 0.f) return pos - ((par.outerRadius - par.innerRadius) * level) * constraint_gradient(par, CC, coarse, pos);
	return pos;
}

// computeSurfaceWaveNormal, :820-867
ST_HD V3 wave_normal(const Par& par, const Cells& CS, const Pts& surf, const float* normals, const float* H, int64_t idx) {
	const V3 pos = pos_of(surf, idx);
	const V3 n = normalized(vec_of(normals, surf.cap, idx));
	V3 t1, t2;
	tangent_frame(n, t1, t2);
	Fit f = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
	ST_NEIGHBOURS_BEGIN(par, CS, surf, pos, par.tangentRadius)
	const V3 q = pos_of(surf, idn);
	int gf = -1;
	V3 g;
	while (gf < 6) {
		gf = ghost_next(par, gf, q, par.tangentRadius, g);
		const float x = dot(g - pos, t1), y = dot(g - pos, t2), z = H[idn];
		fit_add(f, weight_radius(norm(pos - g), par.tangentRadius), x, y, z);
	}
	ST_NEIGHBOURS_END
	const float det = fit_det(f);
	if (det == 0.f) return {0.f, 0.f, 0.f};
	const V3 abc = fit_abc(f, det);
	const V3 vx = {1.f, 0.f, 0.f}, vy = {0.f, 1.f, 0.f}, vz = {0.f, 0.f, 1.f};
	return -normalized(vx * abc.x + vy * abc.y - vz);
}
// computeSurfaceWaveLaplacians, :869-910; waveN[3][n]
ST_HD float wave_laplacian(const Par& par, const Cells& CS, const Pts& surf, const float* normals, const float* H, const float* waveN, int64_t idx) {
	float laplacian = 0.f, wTotal = 0.f;
	const V3 pPos = pos_of(surf, idx), pNormal = vec_of(normals, surf.cap, idx);
	V3 t1, t2;
	tangent_frame(pNormal, t1, t2);
	const V3 wn = vec_of(waveN, surf.n, idx);
	const float ph = H[idx];
	if (wn.z == 0.f) return 0.f;
	ST_NEIGHBOURS_BEGIN(par, CS, surf, pPos, par.tangentRadius)
	const float nh = H[idn];
	const V3 q = pos_of(surf, idn);
	int gf = -1;
	V3 g;
	while (gf < 6) {
		gf = ghost_next(par, gf, q, par.tangentRadius, g);
		const V3 dir = g - pPos;
		const float lengthDir = norm(dir);
		if ((double)lengthDir < 1e-5) continue;
		const V3 tangentDir = lengthDir * normalized(dir - dot(dir, pNormal) * pNormal);
		const float dirX = dot(tangentDir, t1), dirY = dot(tangentDir, t2);
		const float dz = nh - ph - (-wn.x / wn.z) * dirX - (-wn.y / wn.z) * dirY;
		const float w = weight_radius(norm(pPos - g), par.tangentRadius);
		wTotal += w;
		laplacian += clampf(w * 4 * dz / (lengthDir * lengthDir), -100.f, 100.f);
	}
	ST_NEIGHBOURS_END
	return wTotal != 0.f ? laplacian / wTotal : 0.f;
}
// evolveWave, :913-929
ST_HD void evolve_wave(const Par& par, float lap, float seed, float& h, float& dth) {
	dth += par.waveSpeed * par.waveSpeed * par.dt * lap;
	dth /= (1 + par.dt * par.waveDamping);
	h += par.dt * dth;
	h /= (1 + par.dt * par.waveDamping);
	h -= seed;
	dth = clampf(dth, -par.waveMaxFrequency * par.waveMaxAmplitude, par.waveMaxFrequency * par.waveMaxAmplitude);
	h = clampf(h, -par.waveMaxAmplitude, par.waveMaxAmplitude);
}
// computeSurfaceCurvature, :932-958
ST_HD float surface_curvature(const Par& par, const Cells& CS, const Pts& surf, const float* normals, int64_t idx) {
	const V3 pPos = pos_of(surf, idx), pNormal = vec_of(normals, surf.cap, idx);
	float wTotal = 0.f, curv = 0.f;
	ST_NEIGHBOURS_BEGIN(par, CS, surf, pPos, par.normalRadius)
	const V3 q = pos_of(surf, idn), qn = vec_of(normals, surf.cap, idn);
	int gf = -1;
	V3 g;
	while (gf < 6) {
		gf = ghost_next(par, gf, q, par.normalRadius, g);
		const V3 gNormal = ghost_normal(gf, qn);
		const V3 dir = pPos - g;
		if (dot(pNormal, gNormal) < 0.f) continue;
		const float dist = norm(dir);
		if (dist < par.normalRadius / 100.f) continue;
		const float distn = dot(dir, pNormal);
		const float w = weight_radius(dist, par.normalRadius);
		curv += w * distn;
		wTotal += w;
	}
	ST_NEIGHBOURS_END
	if (wTotal != 0.f) curv /= wTotal;
	return fabsf(curv);
}
// smoothCurvature, :961-977; curvIn[n]
ST_HD float smooth_curvature(const Par& par, const Cells& CS, const Pts& surf, const float* curvIn, int64_t idx) {
	const V3 pPos = pos_of(surf, idx);
	float curv = 0.f, wTotal = 0.f;
	ST_NEIGHBOURS_BEGIN(par, CS, surf, pPos, par.normalRadius)
	const float w = weight_radius(norm(pPos - pos_of(surf, idn)), par.normalRadius);
	curv += w * curvIn[idn];
	wTotal += w;
	ST_NEIGHBOURS_END
	if (wTotal != 0.f) curv /= wTotal;
	return curv;
}
// seedWaves, :980-999
ST_HD void seed_wave(const Par& par, float& source, float& seed, float& amp) {
	const float el = par.curvCenter - par.curvRadius, er = par.curvCenter + par.curvRadius;
	const float x = clampf((source - el) / (er - el), 0.f, 1.f);
	const float s = x * x * (3 - 2 * x) * 2.f - 1.f;
	const float maxSeed = par.waveMaxSeedingAmplitude * par.waveMaxAmplitude;
	amp = clampf(amp + s * par.seedStep * maxSeed, 0.f, maxSeed);
	seed = amp * par.costheta;
	source = (s >= 0.f) ? 1.f : 0.f;
}

// ---- host code: the derived parameters of :1086-1092 with the C library's expf / logf / powf and the reference's types ...
static inline Par derive_par(int res, float outerRadius, int surfaceDensity, float dt, float waveSpeed, float waveDamping, float waveSeedFrequency,
                             float waveMaxAmplitude, float waveMaxFrequency, float waveMaxSeedingAmplitude, float curvCenter, float curvRadius,
                             float seedStep, int frameCount) {
	Par p;
	memset(&p, 0, sizeof(p));
	p.res = (float)res;
	p.outerRadius = outerRadius;
	p.innerRadius = (float)((double)outerRadius / 2.0);
	p.meanFineDistance = (float)(M_PI * (double)(p.outerRadius + p.innerRadius) / (double)surfaceDensity);
	// weightKernelCoarseDensity(outer + inner) = exponentialWeight(d, outerRadius, 2.0f): 0 beyond the radius, expf inside it
	const float d = p.outerRadius + p.innerRadius;
	float wk = 0.f;
	if (!(d > p.outerRadius)) {
		const float tmp = d / p.outerRadius;
		wk = expf(-2.0f * tmp * tmp);
	}
	p.constraintA = logf(2.0f / (1.0f + wk)) / (powf((p.outerRadius + p.innerRadius) / 2, 2) - p.innerRadius * p.innerRadius);
	p.normalRadius = 0.5f * (p.outerRadius + p.innerRadius);
	p.tangentRadius = 2.1f * p.meanFineDistance;
	p.bndm = 2.f;
	p.bndp = (float)(res - 2);
	p.dt = dt;
	p.waveSpeed = waveSpeed;
	p.waveDamping = waveDamping;
	p.waveSeedFrequency = waveSeedFrequency;
	p.waveMaxAmplitude = waveMaxAmplitude;
	p.waveMaxFrequency = waveMaxFrequency;
	p.waveMaxSeedingAmplitude = waveMaxSeedingAmplitude;
	p.curvCenter = curvCenter;
	p.curvRadius = curvRadius;
	p.seedStep = seedStep;
	const float theta = dt * frameCount * waveSpeed * waveSeedFrequency;
	p.costheta = cosf(theta);
	p.addRadius = (float)((double)p.meanFineDistance - (1e-6));
	p.delRadius = (float)(0.67 * (double)p.meanFineDistance);
	p.dtheta = 2 * p.meanFineDistance / (p.outerRadius + p.innerRadius);
	return p;
}
// ... and the direction table of initFines (:378-382), i then phi, with the float sin / cos overloads and the fp32 running phi; -> the
// number of directions (the first `cap` are written), -1 beyond 2^20
static inline int64_t direction_table(const Par& p, int64_t cap, float* dirs_host) {
	const unsigned discretization = (unsigned)(3u * (p.outerRadius + p.innerRadius) / p.meanFineDistance);     // (unsigned int) M_PI * ...
	const float dtheta = p.dtheta;
	int64_t count = 0;
	for (unsigned i = 0; i <= discretization / 2; ++i) {
		const float discretization2 = (float)(floor(2 * M_PI * sinf(i * dtheta) / dtheta) + 1);
		for (float phi = 0; phi < 2 * M_PI; phi += (float)(2 * M_PI / discretization2)) {
			const float theta = i * dtheta;
			if (count < cap && dirs_host) {
				dirs_host[3 * count] = sinf(theta) * cosf(phi);
				dirs_host[3 * count + 1] = cosf(theta);
				dirs_host[3 * count + 2] = sinf(theta) * sinf(phi);
			}
			if (++count > (1 << 20)) return -1;
		}
	}
	return count;
}

}  // namespace surfturb
}  // namespace mf
