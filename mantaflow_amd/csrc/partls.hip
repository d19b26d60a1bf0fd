// partls.hip -- the two smooth particle level sets of source/plugin/flip.cpp (include/manta_hip_partls.h):
// averagedParticleLevelset (:476-499) and improvedParticleLevelset (:539-581): ComputeAveragedLevelsetWeight (:366-421),
// correctLevelset (:502-537) with Matrix3x3f::eigenvalues (util/matrixbase.h:184-221), knSmoothGrid / knSmoothGridNeg (:434-474)
// and the final setBound(0.5, 0).  DESIGN.md, "Averaged and improved particle level sets", has the order argument of the gather
// and the fp32 / fp64 map of the eigenvalue routine.
#include "common.h"
#include "../../include/manta_hip_partls.h"

using namespace mf;

namespace {

// fabs(norm(g - p)), vectorbase.h:385-389: 0 up to a squared length of 1e-12, 1 within 1e-12 of 1
__device__ __forceinline__ float dist(float gx, float gy, float gz, float px, float py, float pz) {
	const float dx = gx - px, dy = gy - py, dz = gz - pz;
	const float l = dx * dx + dy * dy + dz * dz;
	const float eps2 = 1e-6f * 1e-6f;
	if (l <= eps2) return 0.f;
	return fabsf((fabs((double)l - 1.) < (double)eps2) ? 1.f : sqrtf(l));
}

// ComputeAveragedLevelsetWeight_ijk, flip.cpp:366-421.  One thread per cell; the cells xj = i-r .. i+r of a row (yj, zj) are
// consecutive entries of the particle index, so one [start, end) range per row visits the particles in the reference's order
// (zj, yj, xj, slot), which is the order of the three fp32 sums.  A cell whose neighbourhood is empty reads the index only.
// The lanes' overlapping row ranges are left to the caches (no LDS staging).
// final: nothing follows but setBound(0.5, 0), which is fused (the border is not gathered).
__global__ void __launch_bounds__(BLOCK)
k_partls_gather(Dim d, int64_t np, int64_t ps, const float* __restrict__ pos, const int32_t* __restrict__ isys, int64_t n_indexed,
                const int32_t* __restrict__ index, float* __restrict__ phi, float* __restrict__ pAcc, float* __restrict__ rAcc,
                float radius, float sradiusInv, const int32_t* __restrict__ ptype, int exclude, int final) {
	CELL_IJK(d)
	if (final && !INTERIOR(d)) {
		phi[idx] = 0.5f;
		return;
	}
	const float gx = (float)i + 0.5f, gy = (float)j + 0.5f, gz = (float)k + 0.5f;
	const int r = (int)radius + 1, rZ = d.is3d ? r : 0;
	float wacc = 0.f, racc = 0.f, pax = 0.f, pay = 0.f, paz = 0.f;
	const int xlo = i - r < 0 ? 0 : i - r, xhi = i + r > d.sx - 1 ? d.sx - 1 : i + r;
	for (int zj = k - rZ; zj <= k + rZ; zj++) {
		if (zj < 0 || zj >= d.sz) continue;
		for (int yj = j - r; yj <= j + r; yj++) {
			if (yj < 0 || yj >= d.sy) continue;
			const int64_t c0 = xlo + d.Y * yj + d.Z * zj, c1 = xhi + d.Y * yj + d.Z * zj;
			const int64_t pStart = index[c0];
			int64_t pEnd = (c1 + 1 < d.n) ? (int64_t)index[c1 + 1] : n_indexed;
			pEnd = pEnd < n_indexed ? pEnd : n_indexed;
			for (int64_t q = pStart < 0 ? 0 : pStart; q < pEnd; q++) {
				const int psrc = isys[q];
				if ((uint64_t)psrc >= (uint64_t)np) continue;
				if (ptype && (ptype[psrc] & exclude)) continue;
				const float px = pos[psrc], py = pos[ps + psrc], pz = pos[2 * ps + psrc];
				const float dx = gx - px, dy = gy - py, dz = gz - pz;
				const float s = (dx * dx + dy * dy + dz * dz) * sradiusInv;
				const double wd = 1. - (double)s;
				const float w = (float)(0. < wd ? wd : 0.);   // std::max(0., 1. - s)
				wacc += w;
				racc += radius * w;
				pax += px * w;
				pay += py * w;
				paz += pz * w;
			}
		}
	}
	float phiv = radius;
	float ox = 0.f, oy = 0.f, oz = 0.f, orr = 0.f;
	if (wacc > 1e-6f) {
		racc /= wacc;
		pax /= wacc;
		pay /= wacc;
		paz /= wacc;
		phiv = dist(gx, gy, gz, pax, pay, paz) - racc;
		ox = pax;
		oy = pay;
		oz = paz;
		orr = racc;
	}
	phi[idx] = phiv;
	if (pAcc) {
		pAcc[idx] = ox;
		pAcc[d.n + idx] = oy;
		pAcc[2 * d.n + idx] = oz;
		rAcc[idx] = orr;
	}
}

// std::max, as the reference nests it: a NaN in the second place is dropped, in the first it stays
__device__ __forceinline__ float std_max(float a, float b) { return (a < b) ? b : a; }

// Matrix3x3f::eigenvalues, util/matrixbase.h:184-221, reduced to max(max(e0, e1), e2).  Every name below is a `Real` of the
// reference and rounds to fp32 where it is assigned; expressions with a double literal are fp64; pow / acos / cos / sin are the
// fp64 functions; std::sqrt(h) has a Real argument (fp32, correctly rounded).
__device__ float max_eigenvalue(float v00, float v01, float v02, float v10, float v11, float v12, float v20, float v21, float v22) {
	const float b = -v00 - v11 - v22;
	const float c = v00 * (v11 + v22) + v11 * v22 - v12 * v21 - v01 * v10 - v02 * v20;
	float dd = -v00 * (v11 * v22 - v12 * v21) - v20 * (v01 * v12 - v11 * v02) - v10 * (v02 * v21 - v22 * v01);
	const float bb = b * b;
	const float f = (float)((3.0 * (double)c - (double)bb) / 3.0);
	const float g = (float)((2.0 * (double)b * (double)b * (double)b - 9.0 * (double)b * (double)c + 27.0 * (double)dd) / 27.0);
	const float gg = g * g, ff = f * f, fff = ff * f;
	const float h = (float)((double)gg / 4.0 + (double)fff / 27.0);
	float e0, e1 = 0.f, e2 = 0.f;
	if (h > 0) {
		const float sh = sqrtf(h);
		float r = (float)((double)(-g) / 2.0 + (double)sh);
		float sign;
		if (r < 0) { r = -r; sign = -1.f; } else sign = 1.f;
		const float s = (float)((double)sign * pow((double)r, 1.0 / 3.0));
		float t = (float)((double)(-g) / 2.0 - (double)sh);
		if (t < 0) { t = -t; sign = -1.f; } else sign = 1.f;
		const float u = (float)((double)sign * pow((double)t, 1.0 / 3.0));
		const float su = s + u;
		e0 = (float)((double)su - (double)b / 3.0);
	} else if (h == 0) {
		if (dd < 0) dd = -dd;   // the reference's sign is +1 on both paths
		e0 = (float)(-1.0 * 1.0 * pow((double)dd, 1.0 / 3.0));
	} else {
		const float ii = (float)sqrt((double)gg / 4.0 - (double)h);
		const float jj = (float)pow((double)ii, 1.0 / 3.0);
		const float kk = (float)acos((double)(-g) / (2.0 * (double)ii));
		const float l = -jj;
		const float m = (float)cos((double)kk / 3.0);
		const float n = (float)(sqrt(3.0) * sin((double)kk / 3.0));
		const float p = (float)((double)(-b) / 3.0);
		e0 = (float)(2e0 * (double)jj * (double)m + (double)p);
		const float mpn = m + n, mmn = m - n;
		e1 = l * mpn + p;
		e2 = l * mmn + p;
	}
	return std_max(std_max(e0, e1), e2);
}

// correctLevelset, flip.cpp:502-537 (KERNEL(bnd=1)); in 2-D d.Z == 0, so the z differences are those of the cell with itself
__global__ void __launch_bounds__(BLOCK)
k_partls_correct(Dim d, float* __restrict__ phi, const float* __restrict__ pAcc, const float* __restrict__ rAcc, float radius, float t_low,
                 float t_high, int final) {
	CELL_IJK(d)
	if (!INTERIOR(d)) {
		if (final) phi[idx] = 0.5f;
		return;
	}
	const float ra = rAcc[idx];
	if (ra <= 1e-6f) return;
	const float *X = pAcc, *Y = pAcc + d.n, *Z = pAcc + 2 * d.n;
	const int64_t sy = d.Y, sz = d.Z;
#define CD(A, o) ((float)(0.5 * (double)(A[idx + (o)] - A[idx - (o)])))
	const float maxEV = max_eigenvalue(CD(X, 1), CD(X, sy), CD(X, sz), CD(Y, 1), CD(Y, sy), CD(Y, sz), CD(Z, 1), CD(Z, sy), CD(Z, sz));
#undef CD
	float corr = 1.f;
	if (maxEV >= t_low) {
		const float t = (t_high - maxEV) / (t_high - t_low);
		corr = t * t * t - 3.f * t * t + 3.f * t;
	}
	if (corr < 0.f) corr = 0.f;
	else if (corr > 1.f) corr = 1.f;
	const float x = dist((float)i + 0.5f, (float)j + 0.5f, (float)k + 0.5f, X[idx], Y[idx], Z[idx]) - ra * corr;
	phi[idx] = (x > radius) ? radius : x;
}

// knSmoothGrid / knSmoothGridNeg, flip.cpp:434-474 (KERNEL(bnd=1)), one pass from `me` into `out`:
//   mode 0  knSmoothGrid into a fresh grid:           out = sum * factor, border 0
//   mode 1  knSmoothGridNeg after a knSmoothGrid:     out holds the grid before that pass; out = v < out ? v : me, border kept
//   mode 2  knSmoothGridNeg into a fresh grid:        out = v < 0 ? v : me, border 0
// final: the pass is the last one and setBound(0.5, 0) follows: the border becomes 0.5
__global__ void __launch_bounds__(BLOCK)
k_partls_smooth(Dim d, const float* __restrict__ me, float* __restrict__ out, float factor, int mode, int final) {
	CELL_IJK(d)
	if (!INTERIOR(d)) {
		if (final) out[idx] = 0.5f;
		else if (mode != 1) out[idx] = 0.f;
		return;
	}
	float v = me[idx] + me[idx + 1] + me[idx - 1] + me[idx + d.Y] + me[idx - d.Y];
	if (d.is3d) {
		const float z = me[idx + d.Z] + me[idx - d.Z];
		v += z;
	}
	v *= factor;
	if (mode != 0) {
		const float t = mode == 1 ? out[idx] : 0.f;
		v = (v < t) ? v : me[idx];
	}
	out[idx] = v;
}

}  // namespace

extern "C" {

int mf_partls_abi_version(void) { return MF_PARTLS_ABI_VERSION; }

int mf_partls_levelset(int sx, int sy, int sz, int64_t np, int64_t pstride, const float* pos, const int32_t* indexSys,
                       int64_t n_indexed, const int32_t* index, float* phi, float radiusFactor, int smoothen, int smoothenNeg,
                       int improved, float t_low, float t_high, const int32_t* ptype, int exclude, float* pAcc, float* rAcc,
                       float* tmp, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("mf_partls_levelset: not available inside a z-slab window");
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	if (smoothen < 0) smoothen = 0;
	if (smoothenNeg < 0) smoothenNeg = 0;
	const int rounds = smoothen > smoothenNeg ? smoothen : smoothenNeg;
	const int passes = smoothen + smoothenNeg;
	if (improved && (!pAcc || !rAcc)) return fail("mf_partls_levelset: the improved form needs pAcc and rAcc");
	if (passes && !tmp) return fail("mf_partls_levelset: smoothing needs tmp");
	if (n_indexed < 0 || n_indexed > np) return fail("mf_partls_levelset: %lld indexed particles of %lld", (long long)n_indexed, (long long)np);
	// calculateRadiusFactor (flip.cpp:198-200) in double, returned as Real; radius = 0.5 * that, rounded to Real
	const float rf = (float)((d.is3d ? sqrt(3.) : sqrt(2.)) * ((double)radiusFactor + .01));
	const float radius = (float)(0.5 * (double)rf);
	const float sradiusInv = (float)(1. / (4. * (double)radius * (double)radius));
	const float factor = (float)(1. / (d.is3d ? 7. : 5.));
	const dim3 grid(nblk(d.n)), block(BLOCK);
	// every pass moves the level set to the other buffer: start where an even number of moves ends in phi
	float* cur = (passes & 1) ? tmp : phi;
	float* oth = (passes & 1) ? phi : tmp;
	hipLaunchKernelGGL(k_partls_gather, grid, block, 0, st, d, np, pstride, pos, indexSys, n_indexed, index, cur, improved ? pAcc : nullptr,
	                   improved ? rAcc : nullptr, radius, sradiusInv, ptype, exclude, (!improved && !passes) ? 1 : 0);
	MF_LAUNCH_CHECK();
	if (improved) {
		hipLaunchKernelGGL(k_partls_correct, grid, block, 0, st, d, cur, pAcc, rAcc, radius, t_low, t_high, passes ? 0 : 1);
		MF_LAUNCH_CHECK();
	}
	int left = passes;
	for (int it = 0; it < rounds; it++) {
		const bool sm = it < smoothen, ng = it < smoothenNeg;
		if (sm) {
			hipLaunchKernelGGL(k_partls_smooth, grid, block, 0, st, d, cur, oth, factor, 0, --left == 0 ? 1 : 0);
			MF_LAUNCH_CHECK();
			float* t = cur; cur = oth; oth = t;
		}
		if (ng) {
			hipLaunchKernelGGL(k_partls_smooth, grid, block, 0, st, d, cur, oth, factor, sm ? 1 : 2, --left == 0 ? 1 : 0);
			MF_LAUNCH_CHECK();
			float* t = cur; cur = oth; oth = t;
		}
	}
	return 0;
}

}  // extern "C"
