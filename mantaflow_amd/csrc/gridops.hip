// gridops.hip -- the grid operations and small grid plugins of include/open/manta_hip_gridops.h: one transposition through LDS, fp64
// reductions in the project's fixed order, and bandwidth-bound element-wise / stencil kernels, one thread per cell (lanes along x).
// Reference: grid.cpp:251-268, 322-348, 387-418, 496-536, 564-571, 717-739, 1013-1033, plugin/extforces.cpp:24-43, 376-407,
// fastmarch.cpp:434-468, 525-557, plugin/initplugins.cpp:110-128, 154-183, plugin/flip.cpp:266-269.
#include "reduce.h"
#include "vec3_math.h"
#include "wavelet_noise_vec.h"
#include "../../include/open/manta_hip_gridops.h"

using namespace mf;
using namespace mf::v3;

namespace {

constexpr int MF_INFLOW = 8, MF_OUTFLOW = 16;   // FlagGrid::TypeInflow, TypeOutflow
constexpr int TILE = MF_GRIDOPS_TILE, PITCH = MF_GRIDOPS_TILE_PITCH;
constexpr int TILE_ROWS = BLOCK / TILE;         // rows of the tile one pass of the 256 threads covers

// ---- knPermuteAxes, grid.cpp:251-256 ----
// axis0 == 0: x stays the fastest axis on both sides.  One thread per SOURCE cell; rows are read and written whole.
// tY / tZ: the target's strides of the axes that source axes y / z go to.
__global__ void __launch_bounds__(BLOCK)
k_permute_rows(Dim d, int ncomp, int64_t tY, int64_t tZ, const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) {
	CELL_IJK(d)
	const int64_t t = (int64_t)i + tY * j + tZ * k;
	for (int c = 0; c < ncomp; c++) dst[c * d.n + t] = src[c * d.n + idx];
}
// axis0 != 0: the target's x is source axis A (1 or 2), the source's x becomes target axis with stride tX, and the remaining source axis
// R (stride sR, extent nR) keeps being a slow axis with target stride tR.  A block moves one TILE x TILE tile of the (x, A) plane of
// one R coordinate and one component: rows of the tile are read along the source's x, columns are written along the target's x.
// tile[r][c] sits at word r * PITCH + c; the column read of lane l is word l * PITCH + c, bank (33 l + c) % 32 = (l + c) % 32:
// 32 different banks for the 32 lanes of a half wavefront.
__global__ void __launch_bounds__(BLOCK)
k_permute_tile(int nx, int nA, int nR, int64_t sA, int64_t sR, int64_t tX, int64_t tR, int64_t n, const uint32_t* __restrict__ src,
               uint32_t* __restrict__ dst) {
	__shared__ uint32_t tile[TILE * PITCH];
	const int tx = threadIdx.x % TILE, ty = threadIdx.x / TILE;
	const int r = blockIdx.z % nR, comp = blockIdx.z / nR;
	const int x0 = blockIdx.x * TILE, a0 = blockIdx.y * TILE;
	const uint32_t* s = src + comp * n + r * sR;
	uint32_t* t = dst + comp * n + r * tR;
#pragma unroll
	for (int q = 0; q < TILE; q += TILE_ROWS) {
		const int x = x0 + tx, a = a0 + ty + q;
		if (x < nx && a < nA) tile[(ty + q) * PITCH + tx] = s[x + a * sA];
	}
	__syncthreads();
#pragma unroll
	for (int q = 0; q < TILE; q += TILE_ROWS) {
		const int a = a0 + tx, x = x0 + ty + q;
		if (x < nx && a < nA) t[a + x * tX] = tile[tx * PITCH + ty + q];
	}
}

// ---- the range of FOR_IJKT_BND / FOR_IJK_BND, kernel.h:39-42, 58-62: z is cut on 3-D grids only ----
struct Range {
	int bnd, rx, ry, rz;
	int64_t m;   // cells in the range; 0 when a side is empty
};
static Range mkrange(const Dim& d, int bnd) {
	Range r;
	r.bnd = bnd;
	r.rx = d.sx - 2 * bnd;
	r.ry = d.sy - 2 * bnd;
	r.rz = d.is3d ? d.sz - 2 * bnd : 1;
	// a negative bnd would walk outside the grid in the reference; the entries refuse it
	r.m = (r.rx > 0 && r.ry > 0 && r.rz > 0) ? (int64_t)r.rx * r.ry * r.rz : 0;
	return r;
}
__device__ __forceinline__ int64_t range_cell(const Dim& d, const Range& r, int64_t q) {
	const unsigned t = (unsigned)q / (unsigned)r.rx;
	const int i = (int)((unsigned)q - t * (unsigned)r.rx) + r.bnd;
	const int j = (int)(t % (unsigned)r.ry) + r.bnd;
	const int k = (int)(t / (unsigned)r.ry) + (d.is3d ? r.bnd : 0);
	return (int64_t)i + (int64_t)d.sx * (j + (int64_t)d.sy * k);
}

// norm(Vector3D<float>), vectorbase.h:385-389: VECTOR_EPSILON is 1e-6f, its square an fp32 product; `l - 1.` is a double expression
__device__ __forceinline__ float norm3(float x, float y, float z) {
	const float l = x * x + y * y + z * z;
	const float eps2 = 1e-6f * 1e-6f;
	if (l <= eps2) return 0.f;
	return (fabs((double)l - 1.) < (double)eps2) ? 1.f : sqrtf(l);
}

// ---- loop_calcL1Grid / loop_calcL2Grid, grid.cpp:390-409: the terms; the sum is fp64 ----
template <int KIND, int L2>
struct NormTerm {
	Dim d;
	Range r;
	const void* a;
	__device__ __forceinline__ void operator()(int64_t q, double (&acc)[1]) const {
		const int64_t idx = range_cell(d, r, q);
		float term;
		if (KIND == 0) {
			const float v = ((const float*)a)[idx];
			term = L2 ? v * v : fabsf(v);
		} else if (KIND == 1) {
			// norm(int) = abs(v), normSquare(int) = square(v) = v * v in int, each converted to Real on return (vectorbase.h:400-401);
			// the product wraps here where the reference's overflows
			const int32_t v = ((const int32_t*)a)[idx];
			term = L2 ? (float)(int32_t)((uint32_t)v * (uint32_t)v) : (float)(v < 0 ? (int32_t)(0u - (uint32_t)v) : v);
		} else {
			const float* f = (const float*)a;
			const float x = f[idx], y = f[d.n + idx], z = f[2 * d.n + idx];
			term = L2 ? x * x + y * y + z * z : norm3(x, y, z);
		}
		acc[0] += (double)term;
	}
};

// ---- knGridTotalSum + knCountFluidCells, grid.cpp:718-725: the sum and the count (exact in fp64) ----
struct AvgTerm {
	const float* a;
	const int32_t* flags;
	__device__ __forceinline__ void operator()(int64_t idx, double (&acc)[2]) const {
		if (flags && !(flags[idx] & MF_FLUID)) return;
		acc[0] += (double)a[idx];
		acc[1] += 1.0;
	}
};

// ---- knJoinReal / knJoinInt / knJoinVec, grid.cpp:258-268: std::max(a, b) is (a < b) ? b : a, std::min(a, b) is (b < a) ? b : a ----
template <class T>
__device__ __forceinline__ T join1(T a, T b, int keepMax) {
	return keepMax ? ((a < b) ? b : a) : ((b < a) ? b : a);
}
template <int KIND>
__global__ void __launch_bounds__(BLOCK) k_join(int64_t n, void* __restrict__ a, const void* __restrict__ b, int keepMax) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	if (KIND == 0) {
		float* x = (float*)a;
		x[idx] = join1(x[idx], ((const float*)b)[idx], keepMax);
	} else if (KIND == 1) {
		int32_t* x = (int32_t*)a;
		x[idx] = join1(x[idx], ((const int32_t*)b)[idx], keepMax);
	} else {
		float* x = (float*)a;
		const float* y = (const float*)b;
		const float ax = x[idx], ay = x[n + idx], az = x[2 * n + idx], bx = y[idx], by = y[n + idx], bz = y[2 * n + idx];
		const float v = join1(ax * ax + ay * ay + az * az, bx * bx + by * by + bz * bz, keepMax);
		x[idx] = v;
		x[n + idx] = v;
		x[2 * n + idx] = v;
	}
}

// the faces KnApplyForceField / KnAddForceIfLower write, extforces.cpp:37-41: the lower neighbour is fluid, or the cell is fluid and the
// lower neighbour empty
__device__ __forceinline__ bool force_face(bool curFluid, int lower) {
	return (lower & MF_FLUID) || (curFluid && (lower & MF_EMPTY));
}

// ---- KnApplyForceField, extforces.cpp:24-43 (KERNEL(bnd = 1)) ----
__global__ void __launch_bounds__(BLOCK)
k_force_field(Dim d, const int32_t* __restrict__ flags, float* __restrict__ vel, const float* __restrict__ force,
              const float* __restrict__ region, int additive, int isMAC) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	const int f = flags[idx];
	const bool curFluid = f & MF_FLUID;
	if (!curFluid && !(f & MF_EMPTY)) return;
	if (region && region[idx] > 0.f) return;
	const int64_t n = d.n;
	const int64_t off[3] = {1, d.Y, d.Z};
	const int nc = d.is3d ? 3 : 2;
	for (int c = 0; c < nc; c++) {
		const float* fc = force + c * n;
		// 0.5 * (a + b): the fp32 sum, halved (the double product rounds to the same fp32)
		const float fv = isMAC ? fc[idx] : 0.5f * (fc[idx - off[c]] + fc[idx]);
		if (force_face(curFluid, flags[idx - off[c]])) vel[c * n + idx] = additive ? vel[c * n + idx] + fv : fv;
	}
}

// ---- KnAddForceIfLower, extforces.cpp:376-402 (KERNEL(bnd = 1)) ----
__global__ void __launch_bounds__(BLOCK)
k_add_force_if_lower(Dim d, const int32_t* __restrict__ flags, float* __restrict__ vel, const float* __restrict__ force) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	const int f = flags[idx];
	const bool curFluid = f & MF_FLUID;
	if (!curFluid && !(f & MF_EMPTY)) return;
	const int64_t n = d.n;
	const int64_t off[3] = {1, d.Y, d.Z};
	const int nc = d.is3d ? 3 : 2;
	for (int c = 0; c < nc; c++) {
		if (!force_face(curFluid, flags[idx - off[c]])) continue;
		const float* fc = force + c * n;
		const float fv = 0.5f * (fc[idx - off[c]] + fc[idx]);
		const float v = vel[c * n + idx];
		const float lo = (fv < v) ? fv : v, hi = (v < fv) ? fv : v;   // std::min(v, fv), std::max(v, fv)
		const float sum = v + fv;
		vel[c * n + idx] = (fv > 0.f) ? ((hi < sum) ? hi : sum) : ((sum < lo) ? lo : sum);   // std::min(sum, max) : std::max(sum, min)
	}
}

// ---- extrapolateVec3Simple, fastmarch.cpp:525-557 ----
// the two serial marking loops in one pass: 1 in the marked interior cells, 2 in the other interior cells next to one
__global__ void __launch_bounds__(BLOCK) k_vec3_mark(Dim d, const float* __restrict__ phi, int32_t* __restrict__ tmp, int inside) {
	CELL_IJK(d)
	int v = 0;
	if (INTERIOR(d)) {
		const float p = phi[idx];
		if (inside ? p > 0.f : p < 0.f) v = 1;
		else {
			const int di[6] = {1, -1, 0, 0, 0, 0}, dj[6] = {0, 0, 1, -1, 0, 0}, dk[6] = {0, 0, 0, 0, 1, -1};
			const int nn = d.is3d ? 6 : 4;
			for (int q = 0; q < nn; q++) {
				const int i2 = i + di[q], j2 = j + dj[q], k2 = k + dk[q];
				// only interior cells are ever marked 1
				if (i2 < 1 || i2 >= d.sx - 1 || j2 < 1 || j2 >= d.sy - 1 || (d.is3d && (k2 < 1 || k2 >= d.sz - 1))) continue;
				const float p2 = phi[idx + di[q] + dj[q] * d.Y + dk[q] * d.Z];
				if (inside ? p2 > 0.f : p2 < 0.f) {
					v = 2;
					break;
				}
			}
		}
	}
	tmp[idx] = v;
}
// knExtrapolateLsSimple<Vec3> with direction = Vec3(0), fastmarch.cpp:439-460.  In place like the reference: a pass only reads cells
// whose marker equals dd and only writes cells whose marker is 0 (to dd + 1), so the result does not depend on the thread order.
__global__ void __launch_bounds__(BLOCK) k_vec3_extrap(Dim d, float* __restrict__ vel, int32_t* __restrict__ tmp, int dd) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	if (tmp[idx] != 0) return;
	const int64_t nb[6] = {1, -1, d.Y, -d.Y, d.Z, -d.Z};
	const int nn = d.is3d ? 6 : 4;
	const int64_t n = d.n;
	int nbs = 0;
	float ax = 0.f, ay = 0.f, az = 0.f;
	for (int q = 0; q < nn; q++)
		if (tmp[idx + nb[q]] == dd) {
			ax += vel[idx + nb[q]];
			ay += vel[n + idx + nb[q]];
			az += vel[2 * n + idx + nb[q]];
			nbs++;
		}
	if (nbs > 0) {
		tmp[idx] = dd + 1;
		const float fn = (float)nbs;
		vel[idx] = ax / fn + 0.f;          // `avg / nbs + direction`: the + 0 turns a -0 into +0
		vel[n + idx] = ay / fn + 0.f;
		vel[2 * n + idx] = az / fn + 0.f;
	}
}
// knSetRemaining<Vec3>, fastmarch.cpp:463-468
__global__ void __launch_bounds__(BLOCK) k_vec3_remaining(Dim d, float* __restrict__ vel, const int32_t* __restrict__ tmp) {
	CELL_IJK(d)
	if (!INTERIOR(d) || tmp[idx] != 0) return;
	vel[idx] = 0.f;
	vel[d.n + idx] = 0.f;
	vel[2 * d.n + idx] = 0.f;
}

// ---- KnApplyEmission, initplugins.cpp:109-122 ----
__global__ void __launch_bounds__(BLOCK)
k_apply_emission(int64_t n, const int32_t* __restrict__ flags, float* __restrict__ target, const float* __restrict__ source,
                 const float* __restrict__ tex, int isAbsolute, int type) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	const int f = flags[idx];
	const bool isInflow = (type & MF_INFLOW) && (f & MF_INFLOW), isOutflow = (type & MF_OUTFLOW) && (f & MF_OUTFLOW);
	if ((type && !isInflow && !isOutflow) && (tex && !(tex[idx] != 0.f))) return;
	target[idx] = isAbsolute ? source[idx] : target[idx] + source[idx];
}

// ---- KnResetInObstacle, initplugins.cpp:154-177 ----
struct ResetGrids {
	float* g[7];   // density, heat, fuel, flame, red, green, blue; the host has cleared flame without fuel, green / blue without red
};
__global__ void __launch_bounds__(BLOCK)
k_reset_in_obstacle(int64_t n, const int32_t* __restrict__ flags, float* __restrict__ vel, ResetGrids G, float value) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	if (!(flags[idx] & MF_OBSTACLE)) return;
	vel[idx] = value;
	vel[n + idx] = value;
	vel[2 * n + idx] = value;
#pragma unroll
	for (int q = 0; q < 7; q++)
		if (G.g[q]) G.g[q][idx] = value;
}

// ---- copyMACData, grid.cpp:1013-1033 ----
__global__ void __launch_bounds__(BLOCK)
k_copy_mac_data(Dim d, Range r, const float* __restrict__ source, float* __restrict__ target, const int32_t* __restrict__ flags, int flag) {
	const int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (q >= r.m) return;
	const int64_t idx = range_cell(d, r, q);
	if (!(flags[idx] & flag)) return;
	target[idx] = source[idx];
	target[d.n + idx] = source[d.n + idx];
	target[2 * d.n + idx] = source[2 * d.n + idx];
}

// ---- knCopyVec3ToReal / knCopyRealToVec3, grid.cpp:516-536, on SoA planes ----
__global__ void __launch_bounds__(BLOCK)
k_copy_planes(int64_t n, const float* __restrict__ s0, const float* __restrict__ s1, const float* __restrict__ s2, float* __restrict__ d0,
              float* __restrict__ d1, float* __restrict__ d2) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	d0[idx] = s0[idx];
	d1[idx] = s1[idx];
	d2[idx] = s2[idx];
}

// ---- knResampleMacToVec3, grid.cpp:496-500 (KERNEL(bnd = 1)) ----
__global__ void __launch_bounds__(BLOCK) k_resample_mac_to_vec3(Dim d, const float* __restrict__ source, float* __restrict__ target) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	float x, y, z;
	get_centered(d, source, idx, x, y, z);
	target[idx] = x;
	target[d.n + idx] = y;
	target[2 * d.n + idx] = z;
}

// ---- swapComponents, grid.cpp:564-571 ----
__global__ void __launch_bounds__(BLOCK) k_swap_components(int64_t n, float* __restrict__ vel, int c1, int c2, int c3) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	const float v[3] = {vel[idx], vel[n + idx], vel[2 * n + idx]};
	vel[idx] = v[c1];
	vel[n + idx] = v[c2];
	vel[2 * n + idx] = v[c3];
}

// ---- debugIntToReal, flip.cpp:266-269 ----
__global__ void __launch_bounds__(BLOCK) k_int_to_real(int64_t n, const int32_t* __restrict__ source, float* __restrict__ dest, float factor) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	dest[idx] = (float)source[idx] * factor;
}

// ---- knApplySimpleNoiseReal / knApplySimpleNoiseVec3, waveletturbulence.cpp:85-116: on fluid cells target += noise(cell centre) * scale
// * factor, left to right in fp32; factor = weight(cell) or 1.  The evaluators are those of addNoise / applyNoiseVec3. ----
template <int VEC>
__global__ void __launch_bounds__(BLOCK)
k_simple_noise(Dim d, const int32_t* __restrict__ flags, float* __restrict__ target, const float* __restrict__ tile, NoiseParams P,
               float scale, const float* __restrict__ weight) {
	CELL_IJK(d)
	if (!(flags[idx] & MF_FLUID)) return;
	const float factor = weight ? weight[idx] : 1.f;
	const float x = (float)i + 0.5f, y = (float)j + 0.5f, z = (float)k + 0.5f;
	if (!VEC) {
		target[idx] += noise_evaluate(P, tile, x, y, z) * scale * factor;
	} else {
		// WaveletNoiseField::evaluateCurl, noisefield.h:387-394
		float d0[3], d1[3], d2[3];
		noise_evaluate_vec(P, tile, x, y, z, 0, d0);
		noise_evaluate_vec(P, tile, x, y, z, 1, d1);
		noise_evaluate_vec(P, tile, x, y, z, 2, d2);
		const float cu[3] = {d0[1] - d1[2], d2[2] - d0[0], d1[0] - d2[1]};
#pragma unroll
		for (int c = 0; c < 3; c++) target[c * d.n + idx] += cu[c] * scale * factor;
	}
}

// ---- the legacy single-potential whitewater plugins, secondaryparticles.cpp:549-706 ----
// One thread per cell, neighbours through the caches, visited x outer, y, z inner: the order of the fp32 sums.  Unlike the combined
// plugin these kernels do not test the neighbour against the grid, and they run z over k - radius .. k + radius on a 2-D grid too: there
// the z stride is 0 (grid.cpp:56, Dim::Z), so those iterations address the one plane again -- with their own z in xj -- and the cell
// meets itself as a neighbour for z != k.  Both are kept.  The reference addresses neighbours linearly and so do we; the only guard is
// the array itself: a neighbour whose words (the cell, and for getCentered its three upper neighbours) lie outside [0, n) is skipped,
// where the reference's read is undefined.
__device__ __forceinline__ bool centre_readable(const Dim& d, int64_t q) { return q >= 0 && q + (d.Z > d.Y ? d.Z : d.Y) < d.n; }
__device__ __forceinline__ V3 scaled_centre(const Dim& d, const float* __restrict__ vel, int64_t q, float scale) {
	V3 c;
	get_centered(d, vel, q, c.x, c.y, c.z);
	return scale * c;
}
// MODE 0: knFlipComputePotentialTrappedAir :551-578; MODE 1: knFlipComputePotentialWaveCrest :616-649.  pot.clear() is the 0 every
// other cell gets.
template <int MODE>
__global__ void __launch_bounds__(BLOCK)
k_legacy_gather(Dim d, float* __restrict__ pot, const int32_t* __restrict__ flags, const float* __restrict__ vel,
                const float* __restrict__ normal, int radius, float h, float tauMin, float tauMax, float scale, int itype, int jtype) {
	CELL_IJK(d)
	float out = 0.f;
	if (INTERIOR(d) && (flags[idx] & itype) && centre_readable(d, idx)) {
		const V3 xi = {scale * (float)i, scale * (float)j, scale * (float)k};
		const V3 vi = scaled_centre(d, vel, idx, scale);
		V3 ni = {0.f, 0.f, 0.f};
		if (MODE == 1) ni = {normal[idx], normal[d.n + idx], normal[2 * d.n + idx]};
		float acc = 0.f;
		for (int x = i - radius; x <= i + radius; x++)
			for (int y = j - radius; y <= j + radius; y++)
				for (int z = k - radius; z <= k + radius; z++) {
					if (x == i && y == j && z == k) continue;
					const int64_t q = (int64_t)x + d.Y * y + d.Z * z;
					if (q < 0 || q >= d.n) continue;
					if (!(flags[q] & jtype)) continue;
					const V3 xj = {scale * (float)x, scale * (float)y, scale * (float)z};
					const V3 xij = xi - xj;
					if (MODE == 0) {
						if (!centre_readable(d, q)) continue;
						const V3 vij = vi - scaled_centre(d, vel, q, scale);
						acc += norm3(vij) * (1.f - dot(normalized(vij), normalized(xij))) * (1.f - norm3(xij) / h);
					} else {
						const V3 nj = {normal[q], normal[d.n + q], normal[2 * d.n + q]};
						if (dot(normalized(xij), ni) < 0.f) acc += (1.f - dot(ni, nj)) * (1.f - norm3(xij) / h);
					}
				}
		if (MODE == 0) out = clamp_potential(acc, tauMin, tauMax);
		else out = ((double)dot(normalized(vi), ni) >= 0.6) ? clamp_potential(acc, tauMin, tauMax) : 0.f;
	}
	pot[idx] = out;
}
// knFlipComputePotentialKineticEnergy :592-603 (KERNEL(): every cell): Real(0.5) * 125 * normSquare(vi)
__global__ void __launch_bounds__(BLOCK)
k_legacy_kinetic(Dim d, float* __restrict__ pot, const int32_t* __restrict__ flags, const float* __restrict__ vel, float tauMin, float tauMax,
                 float scale, int itype) {
	CELL_IJK(d)
	float out = 0.f;
	if ((flags[idx] & itype) && centre_readable(d, idx)) {
		const V3 vi = scaled_centre(d, vel, idx, scale);
		out = clamp_potential(62.5f * (vi.x * vi.x + vi.y * vi.y + vi.z * vi.z), tauMin, tauMax);
	}
	pot[idx] = out;
}
// knFlipUpdateNeighborRatio :674-698: jtype means "skip" here; 0 / 0 is NaN, as in the reference
__global__ void __launch_bounds__(BLOCK)
k_legacy_ratio(Dim d, const int32_t* __restrict__ flags, float* __restrict__ ratio, int radius, int itype, int jtype) {
	CELL_IJK(d)
	float out = 0.f;
	if (INTERIOR(d) && (flags[idx] & itype)) {
		int countFluid = 0, countMaxFluid = 0;
		for (int x = i - radius; x <= i + radius; x++)
			for (int y = j - radius; y <= j + radius; y++)
				for (int z = k - radius; z <= k + radius; z++) {
					if (x == i && y == j && z == k) continue;
					const int64_t q = (int64_t)x + d.Y * y + d.Z * z;
					if (q < 0 || q >= d.n) continue;
					const int f = flags[q];
					if (f & jtype) continue;
					if (f & itype) countFluid++;
					countMaxFluid++;
				}
		out = (float)countFluid / (float)countMaxFluid;
	}
	ratio[idx] = out;
}
// flipComputeSurfaceNormals :662-670: GradientOp (commonkernels.h:67-72) on the interior, then getNormalized in every cell
__global__ void __launch_bounds__(BLOCK) k_surface_normals(Dim d, float* __restrict__ normal, const float* __restrict__ phi) {
	CELL_IJK(d)
	V3 g = {normal[idx], normal[d.n + idx], normal[2 * d.n + idx]};
	if (INTERIOR(d)) {
		g.x = 0.5f * (phi[idx + 1] - phi[idx - 1]);
		g.y = 0.5f * (phi[idx + d.Y] - phi[idx - d.Y]);
		g.z = d.is3d ? 0.5f * (phi[idx + d.Z] - phi[idx - d.Z]) : 0.f;
	}
	g = normalized(g);
	normal[idx] = g.x;
	normal[d.n + idx] = g.y;
	normal[2 * d.n + idx] = g.z;
}

int check_n(const char* who, int64_t n) {
	if (n < 0 || n >= (int64_t)1 << 31) return fail("%s: invalid size %lld", who, (long long)n);
	return 0;
}

template <int KIND>
int reduce_norm(int l2, const Dim& d, const Range& r, const void* a, Workspace* ws, hipStream_t st) {
	const dim3 grid(blocks_for(r.m, BLOCK * 8, 1024));
	const Store<double> out = {(double*)ws->scalars};
	if (l2) return reduce<SumF64, 1>(r.m, grid, NormTerm<KIND, 1>{d, r, a}, ws->partials, out, st);
	return reduce<SumF64, 1>(r.m, grid, NormTerm<KIND, 0>{d, r, a}, ws->partials, out, st);
}

}  // namespace

extern "C" {

int mf_gridops_abi_version(void) { return MF_GRIDOPS_ABI_VERSION; }

int mf_gridops_permute(int sx, int sy, int sz, int axis0, int axis1, int axis2, int ncomp, const void* src, void* dst, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const int ax[3] = {axis0, axis1, axis2};
	int seen = 0;
	for (int q = 0; q < 3; q++) {
		if (ax[q] < 0 || ax[q] > 2) return fail("mf_gridops_permute: invalid axis %d", ax[q]);
		seen |= 1 << ax[q];
	}
	if (seen != 7) return fail("mf_gridops_permute: (%d, %d, %d) is no permutation", axis0, axis1, axis2);
	if (ncomp != 1 && ncomp != 3) return fail("mf_gridops_permute: invalid ncomp %d", ncomp);
	if (src == dst) return fail("mf_gridops_permute: dst must not alias src");
	const int S[3] = {sx, sy, sz};
	const int T[3] = {S[axis0], S[axis1], S[axis2]};
	if (T[0] < 2 || T[1] < 2) return fail("mf_gridops_permute: invalid target size %dx%dx%d", T[0], T[1], T[2]);
	const int64_t n = (int64_t)sx * sy * sz;
	const int64_t tstr[3] = {1, T[0], (int64_t)T[0] * T[1]};   // the target's strides
	const int64_t sstr[3] = {1, sx, (int64_t)sx * sy};
	int64_t ts[3];                                              // the target stride of source axis q
	for (int m = 0; m < 3; m++) ts[ax[m]] = tstr[m];
	const hipStream_t st = (hipStream_t)stream;
	if (axis0 == 0) {
		const Dim d = mkdim(sx, sy, sz);
		hipLaunchKernelGGL(k_permute_rows, dim3(nblk(n)), dim3(BLOCK), 0, st, d, ncomp, ts[1], ts[2], (const uint32_t*)src, (uint32_t*)dst);
	} else {
		const int A = axis0, R = 3 - A;   // {A, R} = {1, 2}
		if ((int64_t)S[R] * ncomp > 65535) return fail("mf_gridops_permute: %d planes are too many for one launch", S[R] * ncomp);
		const dim3 grid((sx + TILE - 1) / TILE, (S[A] + TILE - 1) / TILE, S[R] * ncomp);
		if (grid.y > 65535) return fail("mf_gridops_permute: grid too large");
		hipLaunchKernelGGL(k_permute_tile, grid, dim3(BLOCK), 0, st, sx, S[A], S[R], sstr[A], sstr[R], ts[0], ts[R], n, (const uint32_t*)src,
		                   (uint32_t*)dst);
	}
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_norm(int kind, int l2, int sx, int sy, int sz, int bnd, const void* a, float* result_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (kind < 0 || kind > 2) return fail("mf_gridops_norm: unknown kind %d", kind);
	if (bnd < 0) return fail("mf_gridops_norm: negative bnd %d", bnd);
	const Dim d = mkdim(sx, sy, sz);
	const Range r = mkrange(d, bnd);
	if (r.m == 0) {
		*result_host = 0.f;
		return 0;
	}
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const hipStream_t st = (hipStream_t)stream;
	MF_TRY(kind == 0 ? reduce_norm<0>(l2, d, r, a, ws, st) : kind == 1 ? reduce_norm<1>(l2, d, r, a, ws, st) : reduce_norm<2>(l2, d, r, a, ws, st));
	double acc;
	MF_TRY(read_scalars(ws, ws->scalars, sizeof(double), &acc, st));
	*result_host = l2 ? (float)sqrt(acc) : (float)acc;
	return 0;
}

int mf_gridops_join(int kind, int64_t n, void* a, const void* b, int keepMax, void* stream) {
	MF_TRY(check_n("mf_gridops_join", n));
	if (kind < 0 || kind > 2) return fail("mf_gridops_join: unknown kind %d", kind);
	if (n == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	if (kind == 0) hipLaunchKernelGGL(k_join<0>, dim3(nblk(n)), dim3(BLOCK), 0, st, n, a, b, keepMax);
	else if (kind == 1) hipLaunchKernelGGL(k_join<1>, dim3(nblk(n)), dim3(BLOCK), 0, st, n, a, b, keepMax);
	else hipLaunchKernelGGL(k_join<2>, dim3(nblk(n)), dim3(BLOCK), 0, st, n, a, b, keepMax);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_force_field(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* force, const float* region, int additive,
                           int isMAC, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (vel == force) return fail("mf_gridops_force_field: vel must not alias force");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_force_field, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, vel, force, region, additive, isMAC);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_add_force_if_lower(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* force, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (vel == force) return fail("mf_gridops_add_force_if_lower: vel must not alias force");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_add_force_if_lower, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, vel, force);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_extrapolate_vec3_simple(int sx, int sy, int sz, float* vel, const float* phi, int distance, int inside, int32_t* tmp,
                                       void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	const hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_vec3_mark, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, phi, tmp, inside);
	for (int dd = 2; dd < 1 + distance; dd++) hipLaunchKernelGGL(k_vec3_extrap, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, vel, tmp, dd);
	hipLaunchKernelGGL(k_vec3_remaining, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, vel, tmp);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_apply_emission(int64_t n, const int32_t* flags, float* target, const float* source, const float* emissionTexture,
                              int isAbsolute, int type, void* stream) {
	MF_TRY(check_n("mf_gridops_apply_emission", n));
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_apply_emission, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, flags, target, source, emissionTexture,
	                   isAbsolute, type);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_reset_in_obstacle(int64_t n, const int32_t* flags, float* vel, float* density, float* heat, float* fuel, float* flame,
                                 float* red, float* green, float* blue, float resetValue, void* stream) {
	MF_TRY(check_n("mf_gridops_reset_in_obstacle", n));
	if (fuel && !flame) return fail("mf_gridops_reset_in_obstacle: fuel without flame");
	if (red && (!green || !blue)) return fail("mf_gridops_reset_in_obstacle: red without green and blue");
	if (n == 0) return 0;
	const ResetGrids G = {{density, heat, fuel, fuel ? flame : nullptr, red, red ? green : nullptr, red ? blue : nullptr}};
	hipLaunchKernelGGL(k_reset_in_obstacle, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, flags, vel, G, resetValue);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_copy_mac_data(int sx, int sy, int sz, const float* source, float* target, const int32_t* flags, int flag, int bnd,
                             void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (bnd < 0) return fail("mf_gridops_copy_mac_data: negative bnd %d", bnd);
	const Dim d = mkdim(sx, sy, sz);
	const Range r = mkrange(d, bnd);
	if (r.m == 0) return 0;
	hipLaunchKernelGGL(k_copy_mac_data, dim3(nblk(r.m)), dim3(BLOCK), 0, (hipStream_t)stream, d, r, source, target, flags, flag);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_copy_planes(int64_t n, const float* src0, const float* src1, const float* src2, float* dst0, float* dst1, float* dst2,
                           void* stream) {
	MF_TRY(check_n("mf_gridops_copy_planes", n));
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_copy_planes, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, src0, src1, src2, dst0, dst1, dst2);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_resample_mac_to_vec3(int sx, int sy, int sz, const float* source, float* target, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (source == target) return fail("mf_gridops_resample_mac_to_vec3: target must not alias source");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_resample_mac_to_vec3, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, source, target);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_swap_components(int64_t n, float* vel, int c1, int c2, int c3, void* stream) {
	MF_TRY(check_n("mf_gridops_swap_components", n));
	if (c1 < 0 || c1 > 2 || c2 < 0 || c2 > 2 || c3 < 0 || c3 > 2) return fail("mf_gridops_swap_components: component (%d, %d, %d) outside 0..2", c1, c2, c3);
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_swap_components, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, vel, c1, c2, c3);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_grid_avg(int64_t n, const float* source, const int32_t* flags, float* result_host, void* stream) {
	MF_TRY(check_n("mf_gridops_grid_avg", n));
	if (n == 0) {
		*result_host = -1.f;
		return 0;
	}
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const hipStream_t st = (hipStream_t)stream;
	double r[2];
	MF_TRY((reduce<SumF64, 2>(n, dim3(blocks_for(n, BLOCK * 8, 1024)), AvgTerm{source, flags}, ws->partials, Store<double, 2>{(double*)ws->scalars}, st)));
	MF_TRY(read_scalars(ws, ws->scalars, sizeof(r), r, st));
	// getGridAvg, grid.cpp:736-738: `sum *= 1. / cells`, returned as Real
	*result_host = r[1] > 0. ? (float)(r[0] * (1. / r[1])) : -1.f;
	return 0;
}

int mf_gridops_simple_noise(int vec, int sx, int sy, int sz, const int32_t* flags, float* target, const float* tile, const float* params,
                            float scale, const float* weight, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (!tile || !params) return fail("mf_gridops_simple_noise: no noise tile / parameters");
	const Dim d = mkdim(sx, sy, sz);
	const NoiseParams P = noise_params_vec(params);
	const hipStream_t st = (hipStream_t)stream;
	if (vec) hipLaunchKernelGGL(k_simple_noise<1>, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, flags, target, tile, P, scale, weight);
	else hipLaunchKernelGGL(k_simple_noise<0>, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, flags, target, tile, P, scale, weight);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_legacy_potential(int which, int sx, int sy, int sz, float* pot, const int32_t* flags, const float* vel, const float* normal,
                                int radius, float tauMin, float tauMax, float scaleFromManta, int itype, int jtype, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (which < 0 || which > 2) return fail("mf_gridops_legacy_potential: unknown potential %d", which);
	if (which != 2 && (radius < 0 || radius > 16)) return fail("mf_gridops_legacy_potential: radius %d outside 0..16", radius);
	if (which == 1 && !normal) return fail("mf_gridops_legacy_potential: the wave crest needs the normal grid");
	const Dim d = mkdim(sx, sy, sz);
	const hipStream_t st = (hipStream_t)stream;
	// Real h = !pot.is3D() ? 1.414 * radius : 1.732 * radius: a double product, narrowed
	const float h = (float)((d.is3d ? 1.732 : 1.414) * (double)radius);
	if (which == 0) hipLaunchKernelGGL(k_legacy_gather<0>, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, pot, flags, vel, normal, radius, h, tauMin, tauMax, scaleFromManta, itype, jtype);
	else if (which == 1) hipLaunchKernelGGL(k_legacy_gather<1>, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, pot, flags, vel, normal, radius, h, tauMin, tauMax, scaleFromManta, itype, jtype);
	else hipLaunchKernelGGL(k_legacy_kinetic, dim3(nblk(d.n)), dim3(BLOCK), 0, st, d, pot, flags, vel, tauMin, tauMax, scaleFromManta, itype);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_neighbor_ratio(int sx, int sy, int sz, const int32_t* flags, float* ratio, int radius, int itype, int jtype, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (radius < 0 || radius > 16) return fail("mf_gridops_neighbor_ratio: radius %d outside 0..16", radius);
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_legacy_ratio, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, ratio, radius, itype, jtype);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_surface_normals(int sx, int sy, int sz, float* normal, const float* phi, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_surface_normals, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, normal, phi);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_gridops_int_to_real(int64_t n, const int32_t* source, float* dest, float factor, void* stream) {
	MF_TRY(check_n("mf_gridops_int_to_real", n));
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_int_to_real, dim3(nblk(n)), dim3(BLOCK), 0, (hipStream_t)stream, n, source, dest, factor);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
