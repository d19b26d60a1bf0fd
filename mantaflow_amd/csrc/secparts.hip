// secparts.hip -- the secondary particles of source/plugin/secondaryparticles.cpp (include/manta_hip_secparts.h):
// flipComputeSecondaryParticlePotentials (:24-103, GradientOp commonkernels.h:67-72), flipSampleSecondaryParticles (:105-220),
// flipUpdateSecondaryParticles (:225-447), flipDeleteParticlesInObstacle (:450-476), setFlagsFromLevelset / setMACFromLevelset
// (:512-533).  DESIGN.md, "Secondary particles", has the fp32 / fp64 map, the order-free statement of the sampling loop and the
// error bound of the sampled positions.
#include "common.h"
#include "../../include/manta_hip_secparts.h"
#include "scan.h"
#include "vec3_math.h"
#include <limits.h>

using namespace mf;
using namespace mf::v3;

namespace {

constexpr int PSPRAY_ = 1 << 1, PBUBBLE_ = 1 << 2, PFOAM_ = 1 << 3, PDELETE_ = 1 << 10;

// V3, normalized, norm3, std_min, clamp_potential: vec3_math.h (shared with the legacy single-potential plugins of gridops.hip)
// (int)Real as x86-64 converts it: out of range and NaN give INT_MIN (the device's conversion saturates)
__device__ __forceinline__ int to_int(float v) { return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : INT_MIN; }
// GridBase::isInBounds(Vec3i, bnd), grid.h: a 2-D grid has the plane z == 0 only
__device__ __forceinline__ bool in_bounds(const Dim& d, int x, int y, int z, int bnd) {
	bool r = x >= bnd && y >= bnd && x < d.sx - bnd && y < d.sy - bnd;
	if (d.is3d) r = r && z >= bnd && z < d.sz - bnd;
	else r = r && z == 0;
	return r;
}

// ---- potentials ------------------------------------------------------------------------------------------------------------------
// the streaming pass: clears the outputs, GradientOp on the interior, and the per-cell functions the gather needs of a neighbour
__global__ void __launch_bounds__(BLOCK)
k_secparts_pre(Dim d, float* __restrict__ potTA, float* __restrict__ potWC, float* __restrict__ potKE, float* __restrict__ ratio,
               const int32_t* __restrict__ flags, const float* __restrict__ vel, float* __restrict__ normal, const float* __restrict__ phi,
               float scale, int itype, int jtype, float* __restrict__ sv, float* __restrict__ sn, int32_t* __restrict__ sc) {
	CELL_IJK(d)
	potTA[idx] = 0.f;
	potWC[idx] = 0.f;
	potKE[idx] = 0.f;
	ratio[idx] = 0.f;
	if (i <= 0 || i >= d.sx - 1 || j <= 0 || j >= d.sy - 1 || (d.is3d && (k <= 0 || k >= d.sz - 1))) return;
	V3 g;
	g.x = 0.5f * (phi[idx + 1] - phi[idx - 1]);
	g.y = 0.5f * (phi[idx + d.Y] - phi[idx - d.Y]);
	g.z = d.is3d ? 0.5f * (phi[idx + d.Z] - phi[idx - d.Z]) : 0.f;
	normal[idx] = g.x;
	normal[d.n + idx] = g.y;
	normal[2 * d.n + idx] = g.z;
	V3 c;
	get_centered(d, vel, idx, c.x, c.y, c.z);
	c = scale * c;
	const V3 u = normalized(g);
	sv[idx] = c.x;
	sv[d.n + idx] = c.y;
	sv[2 * d.n + idx] = c.z;
	sn[idx] = u.x;
	sn[d.n + idx] = u.y;
	sn[2 * d.n + idx] = u.z;
	const int f = flags[idx];
	sc[idx] = ((f & itype) ? 1 : 0) | ((f & jtype) ? 2 : 0);
}

// knFlipComputeSecondaryParticlePotentials, :31-91.  One thread per cell, lanes along x; the neighbours are visited x outer, y, z
// inner, which is the order of the two fp32 sums.  Neighbour data comes through the caches (no LDS tile).
__global__ void __launch_bounds__(BLOCK)
k_secparts_gather(Dim d, float* __restrict__ potTA, float* __restrict__ potWC, float* __restrict__ potKE, float* __restrict__ ratio,
                  const float* __restrict__ sv, const float* __restrict__ sn, const int32_t* __restrict__ sc, int radius, float h,
                  float tauMinTA, float tauMaxTA, float tauMinWC, float tauMaxWC, float tauMinKE, float tauMaxKE, float scale) {
	CELL_IJK(d)
	if (i < radius || i >= d.sx - radius || j < radius || j >= d.sy - radius) return;
	if (d.is3d && (k < radius || k >= d.sz - radius)) return;
	if (!(sc[idx] & 1)) return;
	const V3 xi = {scale * (float)i, scale * (float)j, scale * (float)k};
	const V3 vi = {sv[idx], sv[d.n + idx], sv[2 * d.n + idx]};
	const V3 ni = {sn[idx], sn[d.n + idx], sn[2 * d.n + idx]};
	float vdiff = 0.f, kappa = 0.f;
	int countFluid = 0, countMaxFluid = 0;
	const int rz = d.is3d ? radius : 0;
	for (int x = i - radius; x <= i + radius; x++) {
		for (int y = j - radius; y <= j + radius; y++) {
			for (int z = k - rz; z <= k + rz; z++) {
				if ((x == i && y == j && z == k) || !in_bounds(d, x, y, z, 1)) continue;
				const int64_t q = x + d.Y * y + d.Z * z;
				const int cls = sc[q];
				if (cls & 2) continue;
				if (cls & 1) countFluid++;
				countMaxFluid++;
				const V3 xj = {scale * (float)x, scale * (float)y, scale * (float)z};
				const V3 vj = {sv[q], sv[d.n + q], sv[2 * d.n + q]};
				const V3 nj = {sn[q], sn[d.n + q], sn[2 * d.n + q]};
				const V3 xij = xi - xj, vij = vi - vj;
				const V3 uxij = normalized(xij);
				const float fall = 1.f - norm3(xij) / h;
				vdiff += norm3(vij) * (1.f - dot(normalized(vij), uxij)) * fall;
				if (dot(uxij, ni) < 0.f) kappa += (1.f - dot(ni, nj)) * fall;
			}
		}
	}
	ratio[idx] = (float)countFluid / (float)countMaxFluid;
	potTA[idx] = clamp_potential(vdiff, tauMinTA, tauMaxTA);
	potWC[idx] = ((double)dot(normalized(vi), ni) >= 0.6) ? clamp_potential(kappa, tauMinWC, tauMaxWC) : 0.f;
	const float ek = 62.5f * (vi.x * vi.x + vi.y * vi.y + vi.z * vi.z);   // Real(0.5) * 125 * normSquare(vi)
	potKE[idx] = clamp_potential(ek, tauMinKE, tauMaxKE);
}

// ---- sampling --------------------------------------------------------------------------------------------------------------------
// the cylinder centre of entry e (multiple) or the cell corner (single); `c` is the cell
__device__ __forceinline__ void entry_cell(const Dim& d, int multiple, int64_t e, int64_t& c, int& i, int& j, int& k, V3& xi) {
	c = multiple ? (e >> 3) : e;
	i = (int)(c % d.sx);
	j = (int)((c / d.sx) % d.sy);
	k = (int)(c / ((int64_t)d.sx * d.sy));
	xi = {(float)i, (float)j, (float)k};
	if (multiple) {
		// for (Real x = i - radius; x <= i + radius; x += 2 * radius), radius = 0.25: i - 0.25, then that + 0.5
		xi.x = (float)i - 0.25f;
		xi.y = (float)j - 0.25f;
		xi.z = (float)k - 0.25f;
		if (e & 4) xi.x += 0.5f;
		if (e & 2) xi.y += 0.5f;
		if (e & 1) xi.z += 0.5f;
	}
}
__device__ __forceinline__ void entry_potentials(const Dim& d, int multiple, int64_t c, V3 xi, const float* __restrict__ potTA,
                                                 const float* __restrict__ potWC, const float* __restrict__ potKE, float& KE, float& TA,
                                                 float& WC) {
	if (multiple) {
		KE = interpol1(d, potKE, xi.x, xi.y, xi.z);
		TA = interpol1(d, potTA, xi.x, xi.y, xi.z);
		WC = interpol1(d, potWC, xi.x, xi.y, xi.z);
	} else {
		KE = potKE[c];
		TA = potTA[c];
		WC = potWC[c];
	}
}

__global__ void __launch_bounds__(BLOCK)
k_secparts_plan(Dim d, int multiple, int64_t entries, const int32_t* __restrict__ flags, const float* __restrict__ potTA,
                const float* __restrict__ potWC, const float* __restrict__ potKE, float k_ta, float k_wc, float dt, int itype,
                int32_t* __restrict__ nraw, int64_t* __restrict__ poff, int64_t* __restrict__ roff) {
	const int64_t e = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (e >= entries) return;
	int64_t c;
	int i, j, k;
	V3 xi;
	entry_cell(d, multiple, e, c, i, j, k, xi);
	int n = 0;
	if (flags[c] & itype) {
		float KE, TA, WC;
		entry_potentials(d, multiple, c, xi, potTA, potWC, potKE, KE, TA, WC);
		n = to_int(KE * (k_ta * TA + k_wc * WC) * dt);
	}
	const int64_t np = n > 0 ? n : 0;
	nraw[e] = n;
	poff[e] = np;
	roff[e] = 4 * np + ((!multiple && n != 0) ? 3 : 0);
}
__global__ void k_secparts_totals(int multiple, int64_t entries, const int32_t* nraw, const int64_t* poff, const int64_t* roff, int64_t* res) {
	const int n = nraw[entries - 1];
	const int64_t np = n > 0 ? n : 0;
	res[0] = poff[entries - 1] + np;
	res[1] = roff[entries - 1] + 4 * np + ((!multiple && n != 0) ? 3 : 0);
}

__global__ void __launch_bounds__(BLOCK)
k_secparts_emit(Dim d, int multiple, int64_t entries, const float* __restrict__ vel, const float* __restrict__ potTA,
                const float* __restrict__ potWC, const float* __restrict__ potKE, const float* __restrict__ ratio,
                const int32_t* __restrict__ nraw, const int64_t* __restrict__ poff, const int64_t* __restrict__ roff,
                const float* __restrict__ reals, int64_t nreals, int64_t np_old, int64_t total, int64_t ps, float* __restrict__ pos,
                int32_t* __restrict__ pflag, float* __restrict__ v_sec, float* __restrict__ l_sec, float lMin, float lMax, float c_s,
                float c_b, float dt) {
	const int64_t m = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (m >= total) return;
	// the last entry whose first particle is at or before m: entries without particles share their successor's offset
	int64_t lo = 0, hi = entries;
	while (hi - lo > 1) {
		const int64_t mid = (lo + hi) >> 1;
		if (poff[mid] <= m) lo = mid;
		else hi = mid;
	}
	const int64_t e = lo, di = m - poff[e];
	if (di >= nraw[e]) return;
	int64_t c;
	int i, j, k;
	V3 xi;
	entry_cell(d, multiple, e, c, i, j, k, xi);
	float KE, TA, WC;
	entry_potentials(d, multiple, c, xi, potTA, potWC, potKE, KE, TA, WC);
	int64_t rb = roff[e];
	if (rb < 0 || rb + (multiple ? 0 : 3) + 4 * (di + 1) > nreals) return;
	if (!multiple) {
		xi = xi + V3{reals[rb], reals[rb + 1], reals[rb + 2]};   // Vec3(i, j, k) + mRand.getVec3()
		rb += 3;
	}
	rb += 4 * di;
	V3 vi;
	interpol_mac(d, vel, xi.x, xi.y, xi.z, vi.x, vi.y, vi.z);
	const V3 dir = dt * vi;
	const V3 e1 = normalized(V3{dir.z, 0.f, -dir.x});
	const V3 cr = {e1.y * dir.z - e1.z * dir.y, e1.z * dir.x - e1.x * dir.z, e1.x * dir.y - e1.y * dir.x};
	const V3 e2 = normalized(cr);
	const float r = (multiple ? 0.25f : 0.5f) * sqrtf(reals[rb]);
	const float theta = (float)((double)(reals[rb + 1] * 2.f) * M_PI);
	const float h = reals[rb + 2] * norm3(dir);
	const float ct = (float)cos((double)theta), st = (float)sin((double)theta);
	const V3 A = (r * ct) * e1, B = (r * st) * e2;
	V3 xd = ((xi + A) + B) + h * normalized(vi);
	if (!d.is3d) xd.z = 0.f;
	const V3 v = (A + B) + vi;
	const float temp = ((KE + TA) + WC) / 3.f;
	const float l = (float)((double)(((lMax - lMin) * temp) + lMin) + (double)reals[rb + 3] * 0.1);
	const int64_t s = np_old + m;
	pos[s] = xd.x;
	pos[ps + s] = xd.y;
	pos[2 * ps + s] = xd.z;
	v_sec[s] = v.x;
	v_sec[ps + s] = v.y;
	v_sec[2 * ps + s] = v.z;
	l_sec[s] = l;
	const float nr = ratio[c];
	pflag[s] = (nr < c_s) ? PSPRAY_ : ((nr > c_b) ? PBUBBLE_ : PFOAM_);
}

// ---- update ----------------------------------------------------------------------------------------------------------------------
// MACGrid::getCentered of a cell of the grid; a face index past the last row / plane (reached only from the outermost layer, which
// the contract keeps free of itype cells) stays on the cell
__device__ __forceinline__ V3 centered_safe(const Dim& d, const float* __restrict__ vel, int x, int y, int z) {
	const int64_t q = x + d.Y * y + d.Z * z;
	const int64_t qx = x + 1 < d.sx ? q + 1 : q, qy = y + 1 < d.sy ? q + d.Y : q, qz = z + 1 < d.sz ? q + d.Z : q;
	V3 c;
	c.x = 0.5f * (vel[q] + vel[qx]);
	c.y = 0.5f * (vel[d.n + q] + vel[d.n + qy]);
	c.z = d.is3d ? 0.5f * (vel[2 * d.n + q] + vel[2 * d.n + qz]) : 0.f;
	return c;
}
// cubicSpline, :226-233: h2, h3, q, square(q), cubed(q) are Real; the polynomial and the constants are double, narrowed on return
__device__ __forceinline__ float cubic_spline(float h, float l, int dim) {
	const float h2 = h * h, h3 = h2 * h;
	const float c = dim == 3 ? (float)(1e0 / (M_PI * (double)h3)) : (float)(10e0 / (7e0 * M_PI * (double)h2));
	const float q = l / h;
	if ((double)q < 1e0) {
		const float sq = q * q, cu = q * q * q;
		return (float)((double)c * (1e0 - 1.5 * (double)sq + 0.75 * (double)cu));
	}
	if ((double)q < 2e0) {
		const double t = 2e0 - (double)q;
		return (float)((double)c * (0.25 * (t * t * t)));
	}
	return 0.f;
}
// the anti-tunnelling samples ct = 1 .. antitunneling - 1 along dt * u, :258-264: true when one of them is outside or in an obstacle
__device__ __forceinline__ bool tunnels(const Dim& d, const int32_t* __restrict__ flags, V3 p, V3 u, float dt, int antitunneling) {
	for (int ct = 1; ct < antitunneling; ct++) {
		const float f = ((float)ct * (1.f / (float)antitunneling)) * dt;
		const V3 t = p + f * u;
		const int x = to_int(t.x), y = to_int(t.y), z = to_int(t.z);
		if (!in_bounds(d, x, y, z, 0)) return true;
		if (flags[x + d.Y * y + d.Z * z] & MF_OBSTACLE) return true;
	}
	return false;
}

template <bool CUBIC>
__global__ void __launch_bounds__(BLOCK)
k_secparts_update(Dim d, int64_t np, int64_t ps, float* __restrict__ pos, int32_t* __restrict__ pflag, float* __restrict__ v_sec,
                  float* __restrict__ l_sec, const float* __restrict__ f_sec, const int32_t* __restrict__ flags,
                  const float* __restrict__ vel, const float* __restrict__ ratio, int radius, V3 g, float k_b, float k_d, float c_s,
                  float c_b, float dt, int exclude, int antitunneling, int itype, unsigned long long* __restrict__ kills) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= np) return;
	int fl = pflag[p];
	if ((fl & PDELETE_) || (fl & exclude)) return;
	V3 x = {pos[p], pos[ps + p], pos[2 * ps + p]};
	const int i = to_int(x.x), j = to_int(x.y), k = to_int(x.z);
	if (!in_bounds(d, i, j, k, 0)) {
		pflag[p] = fl | PDELETE_;
		atomicAdd(kills, 1ull);
		return;
	}
	const float nr = ratio[i + d.Y * j + d.Z * k];
	V3 v = {v_sec[p], v_sec[ps + p], v_sec[2 * ps + p]};
	const int type = (nr < c_s) ? PSPRAY_ : ((nr > c_b) ? PBUBBLE_ : PFOAM_);
	fl = (fl | type) & ~((PSPRAY_ | PBUBBLE_ | PFOAM_) & ~type);
	V3 u;   // the velocity the particle moves with
	if (type == PFOAM_ || (CUBIC && type == PBUBBLE_)) {
		if (CUBIC) {
			V3 sumN = {0.f, 0.f, 0.f};
			float sumD = 0.f;
			const int rz = d.is3d ? radius : 0;
			const float hs = (float)radius * (d.is3d ? 1.732f : 1.414f);
			for (int xx = i - radius; xx <= i + radius; xx++) {
				for (int yy = j - radius; yy <= j + radius; yy++) {
					for (int zz = k - rz; zz <= k + rz; zz++) {
						if ((xx == i && yy == j && zz == k) || !in_bounds(d, xx, yy, zz, 0)) continue;
						if (!(flags[xx + d.Y * yy + d.Z * zz] & itype)) continue;
						const float len = norm3(x - V3{(float)xx, (float)yy, (float)zz});
						const float w = cubic_spline(hs, len, d.is3d ? 3 : 2);
						const V3 c = centered_safe(d, vel, xx, yy, zz);
						sumN = sumN + V3{c.x * w, c.y * w, c.z * w};
						sumD += w;
					}
				}
			}
			u = sumN / sumD;
		} else {
			interpol_mac(d, vel, x.x, x.y, x.z, u.x, u.y, u.z);
		}
	}
	if (type == PSPRAY_) {
		const V3 f = {f_sec[p], f_sec[ps + p], f_sec[2 * ps + p]};
		v = v + dt * (f + g);   // f / 1 is f
		u = v;
	} else if (type == PBUBBLE_) {
		if (!CUBIC) interpol_mac(d, vel, x.x, x.y, x.z, u.x, u.y, u.z);
		const V3 vj = (u - v) / dt;
		v = v + dt * (k_b * V3{-g.x, -g.y, -g.z} + k_d * vj);
		u = v;
	}
	if (type != PFOAM_) {
		v_sec[p] = v.x;
		v_sec[ps + p] = v.y;
		v_sec[2 * ps + p] = v.z;
	}
	if (tunnels(d, flags, x, u, dt, antitunneling)) {
		pflag[p] = fl | PDELETE_;
		atomicAdd(kills, 1ull);
		return;
	}
	x = x + dt * u;
	pos[p] = x.x;
	pos[ps + p] = x.y;
	pos[2 * ps + p] = x.z;
	const float l = l_sec[p] - dt;
	l_sec[p] = l;
	if (l <= 0.f) {
		fl |= PDELETE_;
		atomicAdd(kills, 1ull);
	}
	pflag[p] = fl;
}

// knFlipDeleteParticlesInObstacle, :451-469
__global__ void __launch_bounds__(BLOCK)
k_secparts_delete(Dim d, int64_t np, int64_t ps, const float* __restrict__ pos, int32_t* __restrict__ pflag,
                  const int32_t* __restrict__ flags, unsigned long long* __restrict__ kills) {
	const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (p >= np) return;
	const int fl = pflag[p];
	if (fl & PDELETE_) return;
	const int i = to_int(pos[p]), j = to_int(pos[ps + p]), k = to_int(pos[2 * ps + p]);
	if (!in_bounds(d, i, j, k, 0) || (flags[i + d.Y * j + d.Z * k] & (MF_OBSTACLE | MF_OUTFLOW))) {
		pflag[p] = fl | PDELETE_;
		atomicAdd(kills, 1ull);
	}
}

__global__ void __launch_bounds__(BLOCK)
k_flags_from_levelset(int64_t n, int32_t* __restrict__ flags, const float* __restrict__ phi, int exclude, int itype) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	if (phi[idx] < 0.f && !(flags[idx] & exclude)) flags[idx] = itype;
}
__global__ void __launch_bounds__(BLOCK)
k_mac_from_levelset(Dim d, float* __restrict__ vel, const float* __restrict__ phi, float cx, float cy, float cz) {
	CELL_IJK(d)
	if (interpol1(d, phi, (float)i, (float)j, (float)k) > 0.f) {
		vel[idx] = cx;
		vel[d.n + idx] = cy;
		vel[2 * d.n + idx] = cz;
	}
}

// the kill counter: a device word of the per-device workspace, read back through its pinned mirror
static int kills_begin(unsigned long long** cnt, hipStream_t st) {
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	*cnt = (unsigned long long*)ws->scalars;
	MF_HIP(hipMemsetAsync(*cnt, 0, sizeof(unsigned long long), st));
	return 0;
}
static int kills_end(unsigned long long* cnt, int64_t* kills_host, hipStream_t st) {
	MF_LAUNCH_CHECK();
	return read_back(kills_host, cnt, sizeof(int64_t), st);
}
static int check_particles(const char* who, int64_t np, int64_t pstride) {
	if (np < 0 || pstride < np) return fail("%s: bad particle range (np %lld, stride %lld)", who, (long long)np, (long long)pstride);
	return 0;
}

}  // namespace

extern "C" {

int mf_secparts_abi_version(void) { return MF_SECPARTS_ABI_VERSION; }

int mf_secparts_potentials(int sx, int sy, int sz, float* potTA, float* potWC, float* potKE, float* neighborRatio, const int32_t* flags,
                           const float* vel, float* normal, const float* phi, int radius, float tauMinTA, float tauMaxTA, float tauMinWC,
                           float tauMaxWC, float tauMinKE, float tauMaxKE, float scaleFromManta, int itype, int jtype, float* sv,
                           float* sn, int32_t* sc, int passes, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("mf_secparts_potentials: not available inside a z-slab window");
	if (radius < 1) return fail("flipComputeSecondaryParticlePotentials: radius %d < 1", radius);
	if (!sv || !sn || !sc) return fail("mf_secparts_potentials: needs its scratch arrays");
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	const dim3 grid(nblk(d.n)), block(BLOCK);
	// Real h = !is3D ? 1.414 * radius : 1.732 * radius
	const float h = (float)(d.is3d ? 1.732 * radius : 1.414 * radius);
	if (passes & 1) {
		hipLaunchKernelGGL(k_secparts_pre, grid, block, 0, st, d, potTA, potWC, potKE, neighborRatio, flags, vel, normal, phi,
		                   scaleFromManta, itype, jtype, sv, sn, sc);
		MF_LAUNCH_CHECK();
	}
	if ((passes & 2) && sx > 2 * radius && sy > 2 * radius && (!d.is3d || sz > 2 * radius)) {
		hipLaunchKernelGGL(k_secparts_gather, grid, block, 0, st, d, potTA, potWC, potKE, neighborRatio, sv, sn, sc, radius, h, tauMinTA,
		                   tauMaxTA, tauMinWC, tauMaxWC, tauMinKE, tauMaxKE, scaleFromManta);
		MF_LAUNCH_CHECK();
	}
	return 0;
}

int mf_secparts_scan_bytes(int64_t entries, int64_t* bytes_host) {
	if (entries <= 0 || entries >= ((int64_t)1 << 31)) return fail("flipSampleSecondaryParticles: %lld plan entries", (long long)entries);
	size_t b = 0;
	MF_TRY(exclusive_sum64_bytes(entries, &b));
	*bytes_host = head_ws_bytes(b);
	return 0;
}

int mf_secparts_sample_plan(int sx, int sy, int sz, int multiple, const int32_t* flags, const float* potTA, const float* potWC,
                            const float* potKE, float k_ta, float k_wc, float dt, int itype, int32_t* nraw, int64_t* poff,
                            int64_t* roff, void* tmp, int64_t tmp_bytes, int64_t* totals_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("mf_secparts_sample_plan: not available inside a z-slab window");
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	const int64_t entries = multiple ? 8 * d.n : d.n;
	int64_t need = 0;
	MF_TRY(mf_secparts_scan_bytes(entries, &need));
	HeadWs t;
	MF_TRY(head_ws_cut("flipSampleSecondaryParticles", tmp, tmp_bytes, need, &t));
	hipLaunchKernelGGL(k_secparts_plan, dim3(nblk(entries)), dim3(BLOCK), 0, st, d, multiple, entries, flags, potTA, potWC, potKE, k_ta,
	                   k_wc, dt, itype, nraw, poff, roff);
	MF_LAUNCH_CHECK();
	MF_TRY(exclusive_sum(t.ws, t.ws_bytes, poff, poff, entries, st));
	MF_TRY(exclusive_sum(t.ws, t.ws_bytes, roff, roff, entries, st));
	hipLaunchKernelGGL(k_secparts_totals, dim3(1), dim3(1), 0, st, multiple, entries, nraw, poff, roff, t.head);
	MF_LAUNCH_CHECK();
	return read_back(totals_host, t.head, 2 * sizeof(int64_t), st);
}

int mf_secparts_sample_emit(int sx, int sy, int sz, int multiple, const float* vel, const float* potTA, const float* potWC,
                            const float* potKE, const float* neighborRatio, const int32_t* nraw, const int64_t* poff,
                            const int64_t* roff, const float* reals, int64_t nreals, int64_t np_old, int64_t total, int64_t pstride,
                            float* pos, int32_t* pflag, float* v_sec, float* l_sec, float lMin, float lMax, float c_s, float c_b,
                            float dt, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("mf_secparts_sample_emit: not available inside a z-slab window");
	if (total <= 0) return 0;
	if (np_old < 0 || pstride < np_old + total)
		return fail("flipSampleSecondaryParticles: particle capacity %lld below %lld", (long long)pstride, (long long)(np_old + total));
	if (np_old + total >= ((int64_t)1 << 31)) return fail("flipSampleSecondaryParticles: too many particles for 32-bit indices");
	const Dim d = mkdim(sx, sy, sz);
	const int64_t entries = multiple ? 8 * d.n : d.n;
	hipLaunchKernelGGL(k_secparts_emit, dim3(nblk(total)), dim3(BLOCK), 0, (hipStream_t)stream, d, multiple, entries, vel, potTA, potWC,
	                   potKE, neighborRatio, nraw, poff, roff, reals, nreals, np_old, total, pstride, pos, pflag, v_sec, l_sec, lMin, lMax,
	                   c_s, c_b, dt);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_secparts_update(int sx, int sy, int sz, int cubic, int64_t np, int64_t pstride, float* pos, int32_t* pflag, float* v_sec,
                       float* l_sec, const float* f_sec, const int32_t* flags, const float* vel, const float* neighborRatio, int radius,
                       float gx, float gy, float gz, float k_b, float k_d, float c_s, float c_b, float dt, int exclude, int antitunneling,
                       int itype, int64_t* kills_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("mf_secparts_update: not available inside a z-slab window");
	MF_TRY(check_particles("flipUpdateSecondaryParticles", np, pstride));
	kills_host[0] = 0;
	if (np == 0) return 0;
	if (cubic && radius < 0) radius = 0;
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	unsigned long long* cnt;
	MF_TRY(kills_begin(&cnt, st));
	const V3 g = {gx, gy, gz};
	if (cubic)
		hipLaunchKernelGGL(k_secparts_update<true>, dim3(nblk(np)), dim3(BLOCK), 0, st, d, np, pstride, pos, pflag, v_sec, l_sec, f_sec,
		                   flags, vel, neighborRatio, radius, g, k_b, k_d, c_s, c_b, dt, exclude, antitunneling, itype, cnt);
	else
		hipLaunchKernelGGL(k_secparts_update<false>, dim3(nblk(np)), dim3(BLOCK), 0, st, d, np, pstride, pos, pflag, v_sec, l_sec, f_sec,
		                   flags, vel, neighborRatio, radius, g, k_b, k_d, c_s, c_b, dt, exclude, antitunneling, itype, cnt);
	return kills_end(cnt, kills_host, st);
}

int mf_secparts_delete_in_obstacle(int sx, int sy, int sz, int64_t np, int64_t pstride, const float* pos, int32_t* pflag,
                                   const int32_t* flags, int64_t* kills_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("mf_secparts_delete_in_obstacle: not available inside a z-slab window");
	MF_TRY(check_particles("flipDeleteParticlesInObstacle", np, pstride));
	kills_host[0] = 0;
	if (np == 0) return 0;
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	unsigned long long* cnt;
	MF_TRY(kills_begin(&cnt, st));
	hipLaunchKernelGGL(k_secparts_delete, dim3(nblk(np)), dim3(BLOCK), 0, st, d, np, pstride, pos, pflag, flags, cnt);
	return kills_end(cnt, kills_host, st);
}

int mf_secparts_flags_from_levelset(int64_t n, int32_t* flags, const float* phi, int exclude, int itype, void* stream) {
	if (n <= 0) return 0;
	hipLaunchKernelGGL(k_flags_from_levelset, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, flags, phi, exclude, itype);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_secparts_mac_from_levelset(int sx, int sy, int sz, float* vel, const float* phi, float cx, float cy, float cz, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("mf_secparts_mac_from_levelset: not available inside a z-slab window");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_mac_from_levelset, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, vel, phi, cx, cy, cz);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
