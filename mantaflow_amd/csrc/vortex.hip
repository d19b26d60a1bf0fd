// vortex.hip -- vortex particles (include/open/manta_hip_vortex.h): the all-pairs velocity sum of VortexKernel with one thread per target
// and the sources staged through LDS in tiles every lane reads at the same address, integratePointSet as one launch per Runge-Kutta
// stage with the position update fused, densityFromLevelset, and the host half of VPseedK41.
// Reference: vortexpart.cpp:24-84, util/integrator.h:26-78, plugin/vortexplugins.cpp:169-189, 298-310, util/vectorbase.h:420-434.
#include "common.h"
#include "../../include/open/manta_hip_vortex.h"
#include <math.h>

using namespace mf;

namespace {

constexpr int WG = 64;        // one wave per workgroup: N is often a few thousand, and a target cannot be split
constexpr int TILE = 256;     // sources per LDS tile
constexpr int PDELETE_BIT = 1 << 10;

// what depends on a source alone, computed once per call (k_prepare)
struct Prep {
	float vx, vy, vz, strength;
	float sigma2;
	int skip, pad0, pad1;
};
// a source as the inner loop reads it
struct Src {
	float px, py, pz, strength;
	float vx, vy, vz, sigma2;
	double cut;
	int skip, pad;
};

// normalize(vortNorm) * scale and square(sigma), vortexpart.cpp:32-37 (normalize(): vectorbase.h:420-434)
__global__ void __launch_bounds__(BLOCK)
k_prepare(int64_t nS, int64_t scap, const int32_t* __restrict__ sflag, const float* __restrict__ vort, const float* __restrict__ sigma, float scale,
          Prep* __restrict__ prep) {
	const int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (s >= nS) return;
	float vx = vort[s], vy = vort[scap + s], vz = vort[2 * scap + s];
	const float l = vx * vx + vy * vy + vz * vz;
	const float eps2 = 1e-6f * 1e-6f;
	float nrm;
	if (fabs((double)l - 1.) < (double)eps2) {
		nrm = 1.f;
	} else if (l > eps2) {
		nrm = sqrtf(l);
		const float fac = (float)(1. / (double)nrm);
		vx *= fac;
		vy *= fac;
		vz *= fac;
	} else {
		vx = vy = vz = 0.f;
		nrm = 0.f;
	}
	Prep P;
	P.vx = vx;
	P.vy = vy;
	P.vz = vz;
	P.strength = nrm * scale;
	const float sg = sigma[s];
	P.sigma2 = sg * sg;
	P.skip = (sflag[s] & PDELETE_BIT) ? 1 : 0;
	P.pad0 = P.pad1 = 0;
	prep[s] = P;
}

enum Step { ST_VELOCITY = 0, ST_EULER, ST_RK2_HALF, ST_FULL, ST_RK4_FIRST, ST_RK4_HALF, ST_RK4_FULL, ST_RK4_LAST };

struct Stage {
	int64_t nT, tcap, nS, scap, ucap;
	const float* tpos;      // the targets' positions of this stage
	const int32_t* tflag;
	int tmask;
	const float* spos;      // the sources' positions of this stage (== tpos for advectSelf)
	const Prep* prep;
	float* out;             // ST_VELOCITY: u [3][ucap]; else the positions after the stage [3][tcap]
	float* x0;
	float* uTotal;
	int step;
};

// VortexKernel's sum for one target and, unless step == ST_VELOCITY, the stage's update of integratePointSet
__global__ void __launch_bounds__(WG) k_stage(Stage a) {
	__shared__ Src tile[TILE];
	const int64_t t = blockIdx.x * (int64_t)WG + threadIdx.x;
	const bool live = t < a.nT;
	float px = 0.f, py = 0.f, pz = 0.f;
	bool sum = false;
	if (live) {
		px = a.tpos[t];
		py = a.tpos[a.tcap + t];
		pz = a.tpos[2 * a.tcap + t];
		sum = (a.tflag[t] & a.tmask) == 0;
	}
	float ux = 0.f, uy = 0.f, uz = 0.f;
	for (int64_t base = 0; base < a.nS; base += TILE) {
		__syncthreads();
		for (int j = threadIdx.x; j < TILE; j += WG) {
			const int64_t s = base + j;
			Src S;
			if (s < a.nS) {
				const Prep P = a.prep[s];
				S.px = a.spos[s];
				S.py = a.spos[a.scap + s];
				S.pz = a.spos[2 * a.scap + s];
				S.strength = P.strength;
				S.vx = P.vx;
				S.vy = P.vy;
				S.vz = P.vz;
				S.sigma2 = P.sigma2;
				S.cut = 6.0 * (double)P.sigma2;
				S.skip = P.skip;
				S.pad = 0;
				tile[j] = S;
			}
		}
		__syncthreads();
		if (!sum) continue;
		const int cnt = (int)(a.nS - base < TILE ? a.nS - base : TILE);
		for (int j = 0; j < cnt; j++) {
			const Src& S = tile[j];
			if (S.skip) continue;
			const float rx = px - S.px, ry = py - S.py, rz = pz - S.pz;
			const float rlen2 = rx * rx + ry * ry + rz * rz;
			const double r2 = (double)rlen2;
			if (r2 > S.cut || r2 < 1e-8) continue;      // the cutoff radius; also a particle's term on itself
			const float rlen = sqrtf(rlen2);
			const float z = rx * S.vx + ry * S.vy + rz * S.vz;
			const float ex = ((ry * S.vz) - (rz * S.vy)) / rlen;
			const float ey = ((rz * S.vx) - (rx * S.vz)) / rlen;
			const float ez = ((rx * S.vy) - (ry * S.vx)) / rlen;
			const float rho2 = rlen2 - z * z;
			float vortex = 0.f;
			if ((double)rho2 > 1e-10) vortex = (float)((double)(S.strength * sqrtf(rho2)) * exp((r2 * -0.5) / (double)S.sigma2));
			ux += vortex * ex;
			uy += vortex * ey;
			uz += vortex * ez;
		}
	}
	if (!live) return;
	const float u[3] = {ux, uy, uz};
	if (a.step == ST_VELOCITY) {
		for (int c = 0; c < 3; c++) a.out[c * a.ucap + t] = u[c];
		return;
	}
	const float x[3] = {px, py, pz};
	const float sixth = (float)(1. / 6.);
	for (int c = 0; c < 3; c++) {
		const int64_t q = c * a.tcap + t;
		float r;
		switch (a.step) {
		case ST_EULER:
			r = x[c] + u[c];
			break;
		case ST_RK2_HALF:
			a.x0[q] = x[c];
			r = x[c] + 0.5f * u[c];
			break;
		case ST_FULL:
			r = a.x0[q] + u[c];
			break;
		case ST_RK4_FIRST:
			a.x0[q] = x[c];
			r = x[c] + 0.5f * u[c];
			a.uTotal[q] = u[c] + u[c];
			break;
		case ST_RK4_HALF:
			r = a.x0[q] + 0.5f * u[c];
			a.uTotal[q] = a.uTotal[q] + 2.f * u[c];
			break;
		case ST_RK4_FULL:
			r = a.x0[q] + u[c];
			a.uTotal[q] = a.uTotal[q] + 2.f * u[c];
			break;
		default:
			r = a.x0[q] + sixth * (a.uTotal[q] + u[c]);
			break;
		}
		a.out[q] = r;
	}
}

// densityFromLevelset, vortexplugins.cpp:298-310
__global__ void __launch_bounds__(BLOCK)
k_density_from_levelset(Dim d, const float* __restrict__ phi, float* __restrict__ density, float value, float sigma) {
	CELL_IJK(d)
	const float ph = phi[idx];
	float r;
	if (i < 2 || j < 2 || k < 2 || i >= d.sx - 2 || j >= d.sy - 2 || k >= d.sz - 2) r = 0.f;
	else if (ph < -sigma) r = value;
	else if (ph > sigma) r = 0.f;
	else {
		const float v = (float)(0.5 * (double)value / (double)sigma * (1.0 - (double)ph));
		r = v < 0.f ? 0.f : (v > value ? value : v);      // clamp(), general.h:137-141
	}
	density[idx] = r;
}

int check_sets(const char* who, int64_t nT, int64_t tcap, int64_t nS, int64_t scap) {
	if (nT < 0 || tcap < nT) return fail("%s: %lld targets in arrays of stride %lld", who, (long long)nT, (long long)tcap);
	if (nS < 0 || scap < nS) return fail("%s: %lld sources in arrays of stride %lld", who, (long long)nS, (long long)scap);
	return 0;
}

int prepare(const char* who, int64_t nS, int64_t scap, const int32_t* sflag, const float* vort, const float* sigma, float scale, void* tmp,
            int64_t tmp_bytes, hipStream_t st) {
	if (nS == 0) return 0;
	if (!tmp || tmp_bytes < (int64_t)sizeof(Prep) * nS) return fail("%s: scratch of %lld bytes, %lld needed", who, (long long)tmp_bytes, (long long)(sizeof(Prep) * nS));
	if ((uintptr_t)tmp % 16) return fail("%s: scratch is not 16-byte aligned", who);
	hipLaunchKernelGGL(k_prepare, dim3(nblk(nS)), dim3(BLOCK), 0, st, nS, scap, sflag, vort, sigma, scale, (Prep*)tmp);
	MF_LAUNCH_CHECK();
	return 0;
}

int launch_stage(const Stage& a, hipStream_t st) {
	hipLaunchKernelGGL(k_stage, dim3((unsigned)((a.nT + WG - 1) / WG)), dim3(WG), 0, st, a);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // namespace

extern "C" {

int mf_vortex_abi_version(void) { return MF_VORTEX_ABI_VERSION; }

int mf_vortex_scratch_bytes(int64_t nS, int64_t* bytes_host) {
	if (nS < 0) return fail("mf_vortex_scratch_bytes: %lld sources", (long long)nS);
	*bytes_host = (int64_t)sizeof(Prep) * nS;
	return 0;
}

int mf_vortex_velocity(int64_t nT, int64_t tcap, const float* tpos, const int32_t* tflag, int tmask, int64_t nS, int64_t scap,
                       const float* spos, const int32_t* sflag, const float* vorticity, const float* sigma, float scale, void* tmp,
                       int64_t tmp_bytes, int64_t ucap, float* u, void* stream) {
	MF_TRY(check_sets("mf_vortex_velocity", nT, tcap, nS, scap));
	if (ucap < nT) return fail("mf_vortex_velocity: %lld targets, u of stride %lld", (long long)nT, (long long)ucap);
	if (nT == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	MF_TRY(prepare("mf_vortex_velocity", nS, scap, sflag, vorticity, sigma, scale, tmp, tmp_bytes, st));
	Stage a = {nT, tcap, nS, scap, ucap, tpos, tflag, tmask, spos, (const Prep*)tmp, u, nullptr, nullptr, ST_VELOCITY};
	return launch_stage(a, st);
}

int mf_vortex_integrate(int64_t nT, int64_t tcap, float* tpos, const int32_t* tflag, int tmask, int64_t nS, int64_t scap,
                        const float* spos, const int32_t* sflag, const float* vorticity, const float* sigma, float scale,
                        int integrationMode, float* pos2, float* x0, float* uTotal, void* tmp, int64_t tmp_bytes, void* stream) {
	if (integrationMode < 0 || integrationMode > 2) return fail("unknown integration type");
	const bool self = spos == tpos;
	if (self && (nS != nT || scap != tcap)) return fail("mf_vortex_integrate: the targets are the sources, but %lld / %lld of them", (long long)nT, (long long)nS);
	MF_TRY(check_sets("mf_vortex_integrate", nT, tcap, nS, scap));
	if (nT == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	MF_TRY(prepare("mf_vortex_integrate", nS, scap, sflag, vorticity, sigma, scale, tmp, tmp_bytes, st));
	static const int steps[3][4] = {{ST_EULER, -1, -1, -1}, {ST_RK2_HALF, ST_FULL, -1, -1}, {ST_RK4_FIRST, ST_RK4_HALF, ST_RK4_FULL, ST_RK4_LAST}};
	float* cur = tpos;
	float* nxt = pos2;
	for (int q = 0; q < 4 && steps[integrationMode][q] >= 0; q++) {
		Stage a = {nT, tcap, nS, scap, 0, cur, tflag, tmask, self ? cur : spos, (const Prep*)tmp, nxt, x0, uTotal, steps[integrationMode][q]};
		MF_TRY(launch_stage(a, st));
		float* h = cur;
		cur = nxt;
		nxt = h;
	}
	if (cur != tpos)      // an odd number of stages (Euler) ends in the other buffer
		for (int c = 0; c < 3; c++) MF_HIP(hipMemcpyAsync(tpos + c * tcap, pos2 + c * tcap, sizeof(float) * nT, hipMemcpyDeviceToDevice, st));
	return 0;
}

int mf_vortex_density_from_levelset(int sx, int sy, int sz, const float* phi, float* density, float value, float sigma, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	if (g_slab_gsz > 0) return fail("densityFromLevelset: not available inside a z-slab window");
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_density_from_levelset, dim3(nblk(d.n)), dim3(BLOCK), 0, (hipStream_t)stream, d, phi, density, value, sigma);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_vortex_seed_k41(int64_t m, float strength, float sigma0, float sigma1, float N, const float* p, const float* dir, float* sigmaOut,
                       float* vortOut) {
	if (m < 0) return fail("VPseedK41: %lld particles", (long long)m);
	const float s0 = powf(sigma0, (float)(-(double)N + 1.0));
	const float s1 = powf(sigma1, (float)(-(double)N + 1.0));
	const double inv = 1. / (-(double)N + 1.0);
	const float ex = (float)(-10. / 6. + (double)N / 2.0);
	const float eps2 = 1e-6f * 1e-6f;
	for (int64_t q = 0; q < m; q++) {
		const float sg = (float)pow((1.0 - (double)p[q]) * (double)s0 + (double)(p[q] * s1), inv);
		float v[3] = {dir[3 * q], dir[3 * q + 1], dir[3 * q + 2]};
		const float l = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
		if (fabs((double)l - 1.) < (double)eps2) {
		} else if (l > eps2) {
			const float fac = (float)(1. / (double)sqrtf(l));
			for (int c = 0; c < 3; c++) v[c] *= fac;
		} else {
			v[0] = v[1] = v[2] = 0.f;
		}
		const float pw = powf(sg, ex);
		sigmaOut[q] = sg;
		for (int c = 0; c < 3; c++) vortOut[3 * q + c] = v[c] * strength * pw;
	}
	return 0;
}

}  // extern "C"
