// pressure.hip -- pressure projection on gfx950: 7-point ApplyMatrix stencil, Laplace matrix / rhs assembly,
// velocity correction (+ ghost fluid) and the device-resident PCG loop (the MIC(0) preconditioner lives in mic.hip).
// Reference: source/conjugategrad.{h,cpp}, source/plugin/pressure.cpp (cited per kernel).
#include "reduce.h"
#include "pressure.h"
#include <float.h>
#include <stdlib.h>
#include <stdio.h>
#include <type_traits>

using namespace mf;

static thread_local int g_last_shortcut[3] = {0, 0, 0};      // what mf_cg_last_shortcut reports
// maxIter <= 0: GridCg::solve (conjugategrad.cpp:302-307) never reaches iterate(), and doInit is only called from there -- pressure and
// the work grids stay untouched; mIterations = 0, mResNorm = 1e20 (constructor, :203), sigma 0
static int cg_no_iterations(float* out_host) {
	out_host[0] = 0.f;
	out_host[1] = 1e20f;
	out_host[2] = 0.f;
	return 0;
}

// =========================================================================================================
// ApplyMatrix, conjugategrad.h:118-151
//   non-fluid: dst = src ; fluid: left-to-right fp32 sum of the 7 products.  28 B/cell of compulsory traffic
//   (flags, src, A0, Ai, Aj, Ak read once + dst written); the +-X/+-Y/+-Z neighbours of src and the -X/-Y/-Z
//   entries of Ai/Aj/Ak are re-reads served by L1/L2 (each XCD owns a contiguous z-range of the grid).
//   Optional fusion: per-block fp64 partial sums of dst*src (GridDotProduct(tmp, search)).
// =========================================================================================================

// v5: every load is issued before anything depends on it (no flags -> operand round trip), each thread owns R
// consecutive y-rows of one x-quad so src[j+-1] / Aj[j-1] are reused from registers, and the +-X neighbours come
// from the adjacent lanes (DPP wave shift) instead of three extra 4-byte-per-lane loads.  Per cell: the 7 products of the
// reference in its order.
__device__ __forceinline__ float wave_shr1(float v) {  // lane l gets lane l-1 (lane 0: unchanged)
	return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1(float v) {  // lane l gets lane l+1 (lane 63: unchanged)
	return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x130, 0xf, 0xf, false));
}
// one fluid cell of ApplyMatrix: the left-to-right fp32 sum of the 7 products (5 in 2-D) in the reference's order -- the cell, its
// -X / +X, -Y / +Y, -Z / +Z neighbours, each with the coefficient that couples it (that of the lower cell of the pair)
template <bool IS3D>
__device__ __forceinline__ float stencil_cell(float s, float a0, float sxm, float aim, float sxp, float ai, float sym, float ajm, float syp,
                                              float aj, float szm, float akm, float szp, float ak) {
	float v = s * a0;
	v = v + sxm * aim;
	v = v + sxp * ai;
	v = v + sym * ajm;
	v = v + syp * aj;
	if (IS3D) {
		v = v + szm * akm;
		v = v + szp * ak;
	}
	return v;
}
// PACKED: flags + Ai + Aj + Ak come as one byte per cell (k_mic_pack: fluid bit, "coefficient is -1" bits; only offered by the
// host when every coefficient is exactly +0 or -1): 5 four-byte loads per thread replace 11 sixteen-byte loads, the values
// are rebuilt exactly and everything after the load section is shared
// Non-temporal accesses (common.h: ld_nt4 / st_nt4) for what ApplyMatrix touches once -- the A0 / Ai / flags loads and the dst store:
// 91 -> 69 us at 256^3 (Aj / Ak too: 78 us, they are re-read as the j-1 / k-1 coefficients) -- and for the thread's own src rows
// (68.2 -> 66.2 us; the z neighbours too: 76.8 us)
// Inside the PCG every vector stream EXCEPT the residual is non-temporal -- search and tmp in ApplyMatrix (own rows, result), tmp in the
// residual update, search / tmp / pressure in the search update; the same in the z-slab kernels -- so that what the MIC sweeps read
// (residual, Aprecond, packed bytes, tmp between the two sweeps) stays in L2 / the memory-side cache across the iteration: 72.3 -> 70.8 ms
// per 256^3 step, --slab 74.6 -> 72.3 ms.  Only the complete set pays (any one of these alone: no difference or slower), and only where
// the vectors do not fit the caches anyway: a run-time flag of the kernels (`nt`), set for systems of more than PCG_NT_CELLS cells (10 Mi:
// the 129-plane window of one rank of two, 8.45 M cells, is 1.2 % faster cached) that are swept whole (a liquid scene whose kernels skip
// most bundles touches a fraction: 23.5 ms per dam-break step cached, 23.9 non-temporal).
constexpr int64_t PCG_NT_CELLS = (int64_t)10 << 20;
template <bool DOT, bool IS3D, int R, bool PACKED>
__global__ void __launch_bounds__(BLOCK)
k_apply_matrix_v5(Dim d, const int32_t* __restrict__ flags, float* __restrict__ dst, const float* __restrict__ src,
                  const float* __restrict__ A0, const float* __restrict__ Ai, const float* __restrict__ Aj,
                  const float* __restrict__ Ak, double* __restrict__ partials, const CgScalars* __restrict__ sc, int jgroups, int tpb,
                  const unsigned char* __restrict__ pack, int dk0, int dk1, bool a0_packed, bool nt, SkipMap skip) {   // DOT covers the planes [dk0, dk1) (a z-slab's own)
	// skip (mf_cg_solve, liquid scenes): where it applies src is known to be zero (k_cg_outside_zero found rhs and the work grids zero there,
	// and every kernel of the iteration keeps it so): dst = src = 0 is there already, nothing to do
	// a0_packed (PACKED only): bits 4-7 of the packed bytes hold the diagonal (k_mic_pack) -- A0 is not read at all, 9 instead of 13 B per cell;
	// nt (DOT, the PCG: only as part of the complete set, PCG_NT_CELLS; outside it always): src rows and dst non-temporal
	if (DOT && sc->done) return;
	const bool nts = !DOT || nt;
	const int qx = d.sx >> 2;
	const int64_t nthr = (int64_t)qx * jgroups * d.sz;
	const int vb0 = xcd_swizzle(blockIdx.x, gridDim.x) * tpb;
	double acc = 0.0;
#pragma unroll 1
	for (int t = 0; t < tpb; t++) {
	const int64_t T0 = (int64_t)(vb0 + t) * BLOCK + threadIdx.x;
	const bool live = T0 < nthr;
	const int64_t T = live ? T0 : nthr - 1;
	const int qi = (int)(T % qx);
	const int64_t rg = T / qx;
	const int j0 = (int)(rg % jgroups) * R;
	const int k = (int)(rg / jgroups);
	// (R divides 8: the rows of a thread lie in one bundle; the lanes this thread exchanges +-X neighbours with work on the same rows)
	// (the quads outside the x-range of the system's non-zero packed bytes are as empty as the empty bundles; the first / last quad
	// inside fetch their outer x-neighbour themselves, the lane next to them has left)
	int q_lo = 0, q_hi = qx;
	if (IS3D && skip.on() && skip.active()) {
		const SkipMap::XRange xq = skip.range(d.sx);
		q_lo = xq.lo >> 2;
		q_hi = xq.hi >> 2;
		if (skip.empty_bundle(j0, k) || qi < q_lo || qi >= q_hi) continue;
	}
	const int lane = threadIdx.x & 63;
	const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
	const int64_t Y = d.Y, Z = d.Z;
	const int64_t row0 = ((int64_t)k * d.sy + j0) * d.sx + 4 * qi;  // flat index of this thread's first quad
	int4 f[R];
	float4 sv[R + 2], ajv[R + 1], a0[R], ai[R], ak[R], akm[R], szm[R], szp[R];
	float sl[R], al[R], sr[R];
	// ---- loads (addresses clamped into the grid; out-of-domain neighbours are zeroed afterwards) ----
	// The +-Y neighbours are flat, as in the reference (src[idx -+ Y]): at j = 0 the last row of the plane before, at j = sy-1 the first
	// row of the plane after, zero only at the ends of the grid.  sv[0] / ajv[0] and sv[R + 1] hold them for the edge rows of a plane;
	// with an odd sy the last thread of a plane has one row, and sv[R + 1] is still the row after it.  The interior loads are unchanged.
	{
		const int jm = (rg > 0) ? -1 : 0;
		sv[0] = *(const float4*)(src + row0 + jm * Y);
		if (PACKED) ajv[0] = unpack_coef<PK_AJ>(*(const unsigned*)(pack + row0 + jm * Y));
		else ajv[0] = *(const float4*)(Aj + row0 + jm * Y);
	}
#pragma unroll
	for (int r = 0; r < R; r++) {
		const int jr = (j0 + r < d.sy) ? r : (d.sy - 1 - j0);
		const int64_t idx = row0 + jr * Y;
		sv[r + 1] = ld4(src + idx, nts);
		unsigned pw = 0;
		if (PACKED) pw = *(const unsigned*)(pack + idx);
		if (PACKED && a0_packed) a0[r] = unpack_a0(pw);
		else a0[r] = ld_nt4(A0 + idx);
		if (PACKED) {
			f[r] = unpack_flags(pw);
			ajv[r + 1] = unpack_coef<PK_AJ>(pw);
			ai[r] = unpack_coef<PK_AI>(pw);
		} else {
			f[r] = ld_nt4i(flags + idx);
			ajv[r + 1] = *(const float4*)(Aj + idx);
			ai[r] = ld_nt4(Ai + idx);
		}
		if (IS3D) {
			const int64_t im = (k > 0) ? idx - Z : idx, ip = (k < d.sz - 1) ? idx + Z : idx;
			if (PACKED) {
				ak[r] = unpack_coef<PK_AK>(pw);
				akm[r] = unpack_coef<PK_AK>(*(const unsigned*)(pack + im));
			} else {
				ak[r] = *(const float4*)(Ak + idx);
				akm[r] = *(const float4*)(Ak + im);
			}
			szm[r] = *(const float4*)(src + im);
			szp[r] = *(const float4*)(src + ip);
		}
	}
	{
		const int jr = (j0 + R < d.sy) ? R : (d.sy - j0 - ((k < d.sz - 1) ? 0 : 1));
		sv[R + 1] = *(const float4*)(src + row0 + jr * Y);
	}
	// ---- +-X neighbours: adjacent lanes hold the adjacent quads of the same row, except at row / wave edges ----
	const bool edge_l = (lane == 0) || (qi == 0) || (qi == q_lo), edge_r = (lane == 63) || (qi == qx - 1) || (qi == q_hi - 1);
#pragma unroll
	for (int r = 0; r < R; r++) {
		const int jr = (j0 + r < d.sy) ? r : (d.sy - 1 - j0);
		const int64_t idx = row0 + jr * Y;
		sl[r] = wave_shr1(sv[r + 1].w);
		al[r] = wave_shr1(ai[r].w);
		sr[r] = wave_shl1(sv[r + 1].x);
		if (edge_l) {
			sl[r] = (idx > 0) ? src[idx - 1] : 0.f;
			if (PACKED) al[r] = (idx > 0) ? pk_coef<PK_AI>(pack[idx - 1]) : 0.f;
			else al[r] = (idx > 0) ? Ai[idx - 1] : 0.f;
		}
		if (edge_r) sr[r] = (idx + 4 < d.n) ? src[idx + 4] : 0.f;
	}
#pragma unroll
	for (int r = 0; r < R; r++) {
		const int j = j0 + r;
		if (j >= d.sy) break;
		const int4 fl = f[r];
		const float4 s = sv[r + 1];
		float4 res = s;
		if ((fl.x | fl.y | fl.z | fl.w) & MF_FLUID) {
			const float4 sym = (j > 0 || k > 0) ? sv[r] : z4, ajm = (j > 0 || k > 0) ? ajv[r] : z4;
			const float4 syp = (j < d.sy - 1) ? sv[r + 2] : (k < d.sz - 1) ? sv[R + 1] : z4, aj = ajv[r + 1];
			float4 zm = z4, am = z4, zp = z4, akc = z4;
			if (IS3D) {
				akc = ak[r];
				if (k > 0) {
					zm = szm[r];
					am = akm[r];
				}
				if (k < d.sz - 1) zp = szp[r];
			}
#define CELL5(c, SL, AL, SR) \
	if (fl.c & MF_FLUID) res.c = stencil_cell<IS3D>(s.c, a0[r].c, SL, AL, SR, ai[r].c, sym.c, ajm.c, syp.c, aj.c, zm.c, am.c, zp.c, akc.c);
			CELL5(x, sl[r], al[r], s.y)
			CELL5(y, s.x, ai[r].x, s.z)
			CELL5(z, s.y, ai[r].y, s.w)
			CELL5(w, s.z, ai[r].z, sr[r])
#undef CELL5
		}
		if (live) {
			st4(dst + row0 + r * Y, res, nts);
			if (DOT && k >= dk0 && k < dk1) acc = dot4(acc, res, s);
		}
	}
	}
	if (DOT) {
		acc = block_sum(acc);
		if (threadIdx.x == 0) partials[blockIdx.x] = acc;
	}
}

// z-march: the packed 3-D ApplyMatrix of a whole grid (no skip map, the dot over all planes).  A thread owns one x-quad of ZM_R
// consecutive y-rows and walks a segment of ZM_L planes with them; it keeps in registers the src quads of its rows at the planes
// k-1, k and k+1 and the Ak coefficients of plane k-1, so that per plane it loads its own rows once (of plane k+2, a whole step ahead
// of their use), the two y-halo rows and the packed words of its rows and of row j0-1 (of plane k+1, issued before plane k is
// computed) -- not the +-Z src rows and the k-1 packed word again, and it decodes its index once per segment, not once per tile.
// Every load and store of a step is issued unconditionally, in straight-line code, with its address clamped into the grid and its
// value replaced where it must not count only when it is used: behind a branch that may or may not issue a memory operation the
// compiler has to wait for ALL outstanding ones (vmcnt(0) -- the first form of this kernel did that at every step and gained nothing
// over v5).  For the same reason no branch per cell or row (every cell is computed, a non-fluid cell selects src), and four steps are
// written out with the roles of the register sets rotating, so that no plane is moved from one set to the next.
// The segments of one XCD are one contiguous z-range (xcd_swizzle); at most ZM_MAX_BLOCKS blocks, hence as many dot partials.
// Per cell the expression of v5 (stencil_cell) on the same operands: flat +-X / +-Y neighbours, non-fluid cells copy src.
constexpr int ZM_L = 16, ZM_R = 2;
constexpr int ZM_MAX_BLOCKS = 512;
template <int R>
struct ZmRest {      // what a thread holds of one plane besides its own src rows, as loaded (zm_fix_rest: as used)
	float4 ym, yp;            // src of the rows j0-1 and j0+R (flat: of the neighbouring plane at the plane's edges)
	unsigned pw[R], pwm;      // packed words of the own rows and of row j0-1
	float sl[R], sr[R];       // the -X / +X neighbours of the quad (used by the lanes at the ends of a row or of the wave)
	unsigned pl[R];           // ... and the packed byte of the -X neighbour
};
template <bool NT, int R>
__device__ __forceinline__ void zm_load_rows(float4 (&s)[R], const Dim& d, const float* __restrict__ src, int64_t row0, int j0) {
#pragma unroll
	for (int r = 0; r < R; r++) {
		const int jr = (j0 + r < d.sy) ? r : (d.sy - 1 - j0);
		s[r] = NT ? ld_nt4(src + row0 + jr * d.Y) : *(const float4*)(src + row0 + jr * d.Y);
	}
}
template <bool A0S, int R>
__device__ __forceinline__ void zm_load_rest(ZmRest<R>& p, float4 (&a0)[R], const Dim& d, const float* __restrict__ src, const float* __restrict__ A0,
                                             const unsigned char* __restrict__ pack, int64_t row0, int j0, int k) {
	const int64_t Y = d.Y;
	const int jm = (k > 0 || j0 > 0) ? -1 : 0;
	const int jp = (j0 + R < d.sy) ? R : (d.sy - j0 - ((k < d.sz - 1) ? 0 : 1));
	p.ym = *(const float4*)(src + row0 + jm * Y);
	p.pwm = *(const unsigned*)(pack + row0 + jm * Y);
	p.yp = *(const float4*)(src + row0 + jp * Y);
#pragma unroll
	for (int r = 0; r < R; r++) {
		const int jr = (j0 + r < d.sy) ? r : (d.sy - 1 - j0);
		const int64_t idx = row0 + jr * Y;
		p.pw[r] = *(const unsigned*)(pack + idx);
		if (A0S) a0[r] = ld_nt4(A0 + idx);
		const int64_t il = (idx > 0) ? idx - 1 : 0, ir = (idx + 4 < d.n) ? idx + 4 : idx;
		p.sl[r] = src[il];
		p.pl[r] = (unsigned)pack[il];
		p.sr[r] = src[ir];
	}
}
// the row before the grid's first and the row behind its last, the cell before the first and the cell behind the last: zero, as are
// their couplings
template <int R>
__device__ __forceinline__ void zm_fix_rest(ZmRest<R>& p, const Dim& d, int64_t row0, int j0, int k) {
	const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
	if (!(k > 0 || j0 > 0)) {
		p.ym = z4;
		p.pwm = 0u;
	}
	if (!(k < d.sz - 1 || j0 + R < d.sy)) p.yp = z4;
#pragma unroll
	for (int r = 0; r < R; r++) {
		const int jr = (j0 + r < d.sy) ? r : (d.sy - 1 - j0);
		const int64_t idx = row0 + jr * d.Y;
		if (!(idx > 0)) {
			p.sl[r] = 0.f;
			p.pl[r] = 0u;
		}
		if (!(idx + 4 < d.n)) p.sr[r] = 0.f;
	}
}
// A0S: the diagonal comes from the A0 array, not from bits 4-7 of the packed bytes (a0_packed of k_apply_matrix_v5 clear); NT: its nt
template <bool DOT, bool A0S, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_apply_matrix_zmarch(Dim d, float* __restrict__ dst, const float* __restrict__ src, const float* __restrict__ A0,
                      const unsigned char* __restrict__ pack, double* __restrict__ partials, const CgScalars* __restrict__ sc, int jgroups,
                      int tpb) {
	constexpr int R = ZM_R, L = ZM_L;
	if (DOT && sc->done) return;
	const unsigned qx = (unsigned)(d.sx >> 2);
	const unsigned per_seg = qx * (unsigned)jgroups;
	const unsigned nthr = per_seg * (unsigned)((d.sz + L - 1) / L);
	const int vb0 = xcd_swizzle(blockIdx.x, gridDim.x) * tpb;
	const int lane = threadIdx.x & 63;
	const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
	const int64_t Y = d.Y, Z = d.Z;
	double acc = 0.0;
#pragma unroll 1
	for (int t = 0; t < tpb; t++) {
		const unsigned T0 = (unsigned)(vb0 + t) * BLOCK + threadIdx.x;
		// (the threads behind the last leave: the lane exchange of a live lane never reads them -- the last thread ends a row, and
		// fetches its +X neighbour -- and every memory operation below stays unconditional for the lanes that are left)
		if (T0 >= nthr) continue;
		const unsigned T = T0;
		const unsigned seg = T / per_seg, in_seg = T - seg * per_seg;
		const unsigned jg = in_seg / qx;
		const int qi = (int)(in_seg - jg * qx), j0 = (int)jg * R;
		const int k0 = (int)seg * L, k1 = (k0 + L < d.sz) ? k0 + L : d.sz;
		// (the lanes this thread exchanges +-X neighbours with work on the same rows of the same planes; at the ends of a row and of
		// the wave the neighbour is the fetched one)
		const bool edge_l = (lane == 0) || (qi == 0), edge_r = (lane == 63) || (qi == (int)qx - 1);
		const int64_t row00 = ((int64_t)k0 * d.sy + j0) * d.sx + 4 * qi;      // flat index of this thread's first quad in plane k0

		// One plane: issue the loads of the rest of plane k + 1 (-> n, a0n) and of the own rows of plane k + 2 (-> s2), both planes
		// clamped into the grid, then compute plane k from the rows sm / s0 / s1 of the planes k - 1 / k / k + 1, the rest c / a0c of
		// plane k and the Ak of plane k - 1 (akm); the Ak of plane k -> ako
		auto step = [&](int k, const float4 (&sm)[R], const float4 (&s0)[R], const float4 (&s1)[R], float4 (&s2)[R], ZmRest<R>& c,
		                ZmRest<R>& n, const float4 (&a0c)[R], float4 (&a0n)[R], const float4 (&akm)[R], float4 (&ako)[R]) __attribute__((always_inline)) {
			const int64_t row0 = row00 + (int64_t)(k - k0) * Z;
			const int kn = (k + 1 < d.sz) ? k + 1 : d.sz - 1, k2 = (k + 2 < d.sz) ? k + 2 : d.sz - 1;
			zm_load_rest<A0S, R>(n, a0n, d, src, A0, pack, row00 + (int64_t)(kn - k0) * Z, j0, kn);
			zm_load_rows<NT, R>(s2, d, src, row00 + (int64_t)(k2 - k0) * Z, j0);
			zm_fix_rest<R>(c, d, row0, j0, k);
			const bool top = k == d.sz - 1;
			float4 aj[R + 1], res[R];
			aj[0] = unpack_coef<PK_AJ>(c.pwm);
#pragma unroll
			for (int r = 0; r < R; r++) {
				const unsigned pw = c.pw[r];
				const float4 s = s0[r], ai = unpack_coef<PK_AI>(pw), akc = unpack_coef<PK_AK>(pw);
				aj[r + 1] = unpack_coef<PK_AJ>(pw);
				ako[r] = akc;
				float sl = wave_shr1(s.w), sr = wave_shl1(s.x);
				// (the -X neighbour's "Ai is -1" bit: byte 3 of the word of the lane before)
				float al = pk_coef<(PK_AI << 24)>(__float_as_uint(wave_shr1(__uint_as_float(pw))));
				if (edge_l) {
					sl = c.sl[r];
					al = pk_coef<PK_AI>(c.pl[r]);
				}
				if (edge_r) sr = c.sr[r];
				const float4 a0 = A0S ? a0c[r] : unpack_a0(pw);
				const float4 sym = (r == 0) ? c.ym : s0[r > 0 ? r - 1 : 0], ajm = aj[r];
				const float4 syp = (r + 1 < R) ? ((j0 + r < d.sy - 1) ? s0[r + 1 < R ? r + 1 : 0] : c.yp) : c.yp, ajc = aj[r + 1];
				const float4 zm = sm[r], am = akm[r], zp = top ? z4 : s1[r];
				// (computed for every cell, then selected: no branch per cell)
#define CELL5(c_, BYTE, SL, AL, SR)                                                                                                             \
	{                                                                                                                                       \
		const float v = stencil_cell<true>(s.c_, a0.c_, SL, AL, SR, ai.c_, sym.c_, ajm.c_, syp.c_, ajc.c_, zm.c_, am.c_, zp.c_, akc.c_); \
		res[r].c_ = (pw & (PK_FLUID << (8 * BYTE))) ? v : s.c_;                                                                             \
	}
				CELL5(x, 0, sl, al, s.y)
				CELL5(y, 1, s.x, ai.x, s.z)
				CELL5(z, 2, s.y, ai.y, s.w)
				CELL5(w, 3, s.z, ai.z, sr)
#undef CELL5
				if (DOT && j0 + r < d.sy) acc = dot4(acc, res[r], s);
			}
			// (a row behind the plane's last -- odd sy -- stores the thread's first row again)
#pragma unroll
			for (int r = 0; r < R; r++) {
				const bool own = j0 + r < d.sy;
				const float4 o = own ? res[r] : res[0];
				float* const p = dst + row0 + (own ? r : 0) * Y;
				if (NT) st_nt4(p, o);
				else *(float4*)p = o;
			}
		};

		// ---- the state of plane k0: src rows and Ak of the plane before (zero below the grid), plane k0 whole, src rows of k0 + 1 ----
		float4 sa[R], sb[R], sc_[R], sd[R], a0a[R], a0b[R], aka[R], akb[R];
		ZmRest<R> ca, cb;
#pragma unroll
		for (int r = 0; r < R; r++) sa[r] = aka[r] = z4;
		zm_load_rows<NT, R>(sb, d, src, row00, j0);
		zm_load_rest<A0S, R>(ca, a0a, d, src, A0, pack, row00, j0, k0);
		zm_load_rows<NT, R>(sc_, d, src, row00 + ((k0 + 1 < d.sz) ? Z : 0), j0);
		if (k0 > 0) {
			zm_load_rows<false, R>(sa, d, src, row00 - Z, j0);
#pragma unroll
			for (int r = 0; r < R; r++) {
				const int jr = (j0 + r < d.sy) ? r : (d.sy - 1 - j0);
				aka[r] = unpack_coef<PK_AK>(*(const unsigned*)(pack + row00 - Z + jr * Y));
			}
		}
#pragma unroll 1
		for (int k = k0; k < k1; k += 4) {
			step(k, sa, sb, sc_, sd, ca, cb, a0a, a0b, aka, akb);
			if (k + 1 >= k1) break;
			step(k + 1, sb, sc_, sd, sa, cb, ca, a0b, a0a, akb, aka);
			if (k + 2 >= k1) break;
			step(k + 2, sc_, sd, sa, sb, ca, cb, a0a, a0b, aka, akb);
			if (k + 3 >= k1) break;
			step(k + 3, sd, sa, sb, sc_, cb, ca, a0b, a0a, akb, aka);
		}
	}
	if (DOT) {
		acc = block_sum(acc);
		if (threadIdx.x == 0) partials[blockIdx.x] = acc;
	}
}

// generic fallback (sx % 4 != 0 or unaligned views): one cell per thread
template <bool DOT>
__global__ void __launch_bounds__(BLOCK)
k_apply_matrix_scalar(Dim d, const int32_t* __restrict__ flags, float* __restrict__ dst, const float* __restrict__ src,
                      const float* __restrict__ A0, const float* __restrict__ Ai, const float* __restrict__ Aj,
                      const float* __restrict__ Ak, double* __restrict__ partials, const CgScalars* __restrict__ sc) {
	if (DOT && sc->done) return;
	double acc = 0.0;
	for (int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x; idx < d.n; idx += (int64_t)gridDim.x * BLOCK) {
		const float s = src[idx];
		float v = s;
		if (flags[idx] & MF_FLUID) {
			const int64_t Y = d.Y, Z = d.Z;
			v = s * A0[idx];
			v = v + ((idx >= 1) ? src[idx - 1] * Ai[idx - 1] : 0.f);
			v = v + ((idx + 1 < d.n) ? src[idx + 1] : 0.f) * Ai[idx];
			v = v + ((idx >= Y) ? src[idx - Y] * Aj[idx - Y] : 0.f);
			v = v + ((idx + Y < d.n) ? src[idx + Y] : 0.f) * Aj[idx];
			if (d.is3d) {
				v = v + ((idx >= Z) ? src[idx - Z] * Ak[idx - Z] : 0.f);
				v = v + ((idx + Z < d.n) ? src[idx + Z] : 0.f) * Ak[idx];
			}
		}
		dst[idx] = v;
		if (DOT) {
			const float p = v * s;
			acc += (double)p;
		}
	}
	if (DOT) {
		acc = block_sum(acc);
		if (threadIdx.x == 0) partials[blockIdx.x] = acc;
	}
}


// what ApplyMatrix may use beyond the four coefficient grids (every field optional)
struct AmOpts {
	const unsigned char* pack = nullptr;     // packed bytes of these grids (k_mic_pack) instead of flags / Ai / Aj / Ak
	bool a0_packed = false;                  // ... that carry A0 in bits 4-7 as well
	int dk0 = 0, dk1 = 0x7fffffff;           // DOT: the planes [dk0, dk1) only (a z-slab's own)
	SkipMap skip;                            // liquid scenes (mf_cg_solve): what to leave out
	int nt = -1;                             // DOT: non-temporal vector streams -- 1 on, 0 off, -1 by size (PCG_NT_CELLS)
};
// *nblocks: the number of blocks launched (== number of partials written when DOT); *ranged: DOT honoured dk0 / dk1
template <bool DOT>
static int launch_apply_matrix(const Dim& d, const int32_t* flags, float* dst, const float* src, const float* A0,
                               const float* Ai, const float* Aj, const float* Ak, double* partials,
                               const CgScalars* sc, hipStream_t st, const AmOpts& o = AmOpts{}, int* nblocks = nullptr, bool* ranged = nullptr) {
	if (ranged) *ranged = false;
	const bool nt = !DOT || (o.nt < 0 ? d.n > PCG_NT_CELLS : o.nt != 0);      // (outside the PCG always non-temporal)
	const bool vec = (d.sx % 4 == 0) && al16(flags) && al16(dst) && al16(src) && al16(A0) && al16(Ai) && al16(Aj) && al16(Ak);
	int nb;
	if (vec && d.is3d && o.pack && !o.skip.on() && o.dk0 <= 0 && o.dk1 >= d.sz) {
		// whole packed 3-D grids: the z-marching kernel (the skip map of liquid scenes and the z-slab windows stay on v5)
		const int jgroups = (d.sy + ZM_R - 1) / ZM_R;
		const int64_t vblocks = ((int64_t)(d.sx >> 2) * jgroups * ((d.sz + ZM_L - 1) / ZM_L) + BLOCK - 1) / BLOCK;
		const int tpb = (int)((vblocks + ZM_MAX_BLOCKS - 1) / ZM_MAX_BLOCKS);
		nb = (int)((vblocks + tpb - 1) / tpb);
		const bool a0s = !o.a0_packed;
		auto kern = nt ? (a0s ? k_apply_matrix_zmarch<DOT, true, true> : k_apply_matrix_zmarch<DOT, false, true>)
		               : (a0s ? k_apply_matrix_zmarch<DOT, true, !DOT> : k_apply_matrix_zmarch<DOT, false, !DOT>);
		hipLaunchKernelGGL(kern, dim3(nb), dim3(BLOCK), 0, st, d, dst, src, A0, o.pack, partials, sc, jgroups, tpb);
		if (ranged) *ranged = true;
	} else if (vec) {
		constexpr int R = 2;     // y-rows per thread
		const int jgroups = (d.sy + R - 1) / R;
		const int64_t vblocks = ((int64_t)(d.sx >> 2) * jgroups * d.sz + BLOCK - 1) / BLOCK;
		const int tpb = (int)((vblocks + MAX_BLOCKS - 1) / MAX_BLOCKS);
		nb = (int)((vblocks + tpb - 1) / tpb);
		auto kern = !d.is3d ? k_apply_matrix_v5<DOT, false, R, false> : o.pack ? k_apply_matrix_v5<DOT, true, R, true> : k_apply_matrix_v5<DOT, true, R, false>;
		hipLaunchKernelGGL(kern, dim3(nb), dim3(BLOCK), 0, st, d, flags, dst, src, A0, Ai, Aj, Ak, partials, sc, jgroups, tpb, o.pack, o.dk0, o.dk1, o.a0_packed,
		                   nt, o.skip);
		if (ranged) *ranged = true;
	} else {
		nb = blocks_for(d.n, BLOCK, 2048);
		hipLaunchKernelGGL((k_apply_matrix_scalar<DOT>), dim3(nb), dim3(BLOCK), 0, st, d, flags, dst, src, A0, Ai, Aj, Ak, partials, sc);
	}
	MF_LAUNCH_CHECK();
	if (nblocks) *nblocks = nb;
	return 0;
}

// =========================================================================================================
// assembly kernels (one thread per cell, bnd = 1 unless noted)
// =========================================================================================================
// MakeLaplaceMatrix, conjugategrad.h:154-187
__global__ void __launch_bounds__(BLOCK)
k_make_laplace(Dim d, const int32_t* __restrict__ flags, float* __restrict__ A0, float* __restrict__ Ai,
               float* __restrict__ Aj, float* __restrict__ Ak, const float* __restrict__ fr) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	if (!(flags[idx] & MF_FLUID)) return;
	const int64_t Y = d.Y, Z = d.Z;
	float a0 = A0[idx];
	if (!fr) {
		// `A0 += 1.` : fp32 value + double literal, rounded back; exact for these magnitudes
		if (!(flags[idx - 1] & MF_OBSTACLE)) a0 = (float)((double)a0 + 1.);
		if (!(flags[idx + 1] & MF_OBSTACLE)) a0 = (float)((double)a0 + 1.);
		if (!(flags[idx - Y] & MF_OBSTACLE)) a0 = (float)((double)a0 + 1.);
		if (!(flags[idx + Y] & MF_OBSTACLE)) a0 = (float)((double)a0 + 1.);
		if (d.is3d && !(flags[idx - Z] & MF_OBSTACLE)) a0 = (float)((double)a0 + 1.);
		if (d.is3d && !(flags[idx + Z] & MF_OBSTACLE)) a0 = (float)((double)a0 + 1.);
		if (flags[idx + 1] & MF_FLUID) Ai[idx] = -1.f;
		if (flags[idx + Y] & MF_FLUID) Aj[idx] = -1.f;
		if (d.is3d && (flags[idx + Z] & MF_FLUID)) Ak[idx] = -1.f;
	} else {
		const float *fx = fr, *fy = fr + d.n, *fz = fr + 2 * d.n;
		a0 += fx[idx];
		a0 += fx[idx + 1];
		a0 += fy[idx];
		a0 += fy[idx + Y];
		if (d.is3d) a0 += fz[idx];
		if (d.is3d) a0 += fz[idx + Z];
		if (flags[idx + 1] & MF_FLUID) Ai[idx] = -fx[idx + 1];
		if (flags[idx + Y] & MF_FLUID) Aj[idx] = -fy[idx + Y];
		if (d.is3d && (flags[idx + Z] & MF_FLUID)) Ak[idx] = -fz[idx + Z];
	}
	A0[idx] = a0;
}

// ghost-fluid helpers, plugin/pressure.cpp:115-133, 191-196
__device__ __forceinline__ float thetaHelper(float inside, float outside) {
	const float denom = inside - outside;
	if ((double)denom > -1e-04) return 0.5f;
	const float q = inside / denom;
	const float m = q < 1.f ? q : 1.f;
	return 0.f < m ? m : 0.f;
}
__device__ __forceinline__ float ghostFluidHelper(int64_t idx, int64_t offset, const float* __restrict__ phi, float gfClamp) {
	const float alpha = thetaHelper(phi[idx], phi[idx + offset]);
	if (alpha < gfClamp) return gfClamp;
	return (float)(1. - (1. / (double)alpha));
}
__device__ __forceinline__ float surfTensHelper(int64_t idx, int64_t offset, const float* __restrict__ phi,
                                                const float* __restrict__ curv, float surfTens, float gfClamp) {
	return surfTens * (curv[idx + offset] - ghostFluidHelper(idx, offset, phi, gfClamp) * curv[idx]);
}
__device__ __forceinline__ bool ghostFluidWasClamped(int64_t idx, int64_t offset, const float* __restrict__ phi, float gfClamp) {
	return thetaHelper(phi[idx], phi[idx + offset]) < gfClamp;
}

// MakeRhs, plugin/pressure.cpp:32-84 ; partials[b] = fp64 sum of `set`, partials[MAX_BLOCKS + b] = count
__global__ void __launch_bounds__(BLOCK)
k_make_rhs(Dim d, const int32_t* __restrict__ flags, float* __restrict__ rhs, const float* __restrict__ vel,
           const float* __restrict__ pcc, const float* __restrict__ fr, const float* __restrict__ ob,
           const float* __restrict__ phi, const float* __restrict__ curv, float surfTens, float gfClamp,
           double* __restrict__ partials) {
	double mysum = 0.0, mycnt = 0.0;
	const int64_t X = 1, Y = d.Y, Z = d.Z, n = d.n;
	const float *vx = vel, *vy = vel + n, *vz = vel + 2 * n;
	for (int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * BLOCK) {
		const int i = (int)(idx % d.sx);
		const int j = (int)((idx / d.sx) % d.sy);
		const int k = (int)(idx / ((int64_t)d.sx * d.sy));
		if (!INTERIOR(d)) continue;
		if (!(flags[idx] & MF_FLUID)) {
			rhs[idx] = 0.f;
			continue;
		}
		float set;
		if (!fr) {
			set = vx[idx] - vx[idx + X] + vy[idx] - vy[idx + Y];
			if (d.is3d) set += vz[idx] - vz[idx + Z];
		} else {
			const float *fx = fr, *fy = fr + n, *fz = fr + 2 * n;
			set = fx[idx] * vx[idx] - fx[idx + X] * vx[idx + X] + fy[idx] * vy[idx] - fy[idx + Y] * vy[idx + Y];
			if (d.is3d) set += fz[idx] * vz[idx] - fz[idx + Z] * vz[idx + Z];
			if (ob) {
				const float *ox = ob, *oy = ob + n, *oz = ob + 2 * n;
				set += (1 - fx[idx]) * ox[idx] - (1 - fx[idx + X]) * ox[idx + X] + (1 - fy[idx]) * oy[idx] -
				       (1 - fy[idx + Y]) * oy[idx + Y];
				if (d.is3d) set += (1 - fz[idx]) * oz[idx] - (1 - fz[idx + Z]) * oz[idx + Z];
			}
		}
		if (phi && curv) {
			if (flags[idx - X] & MF_EMPTY) set += surfTensHelper(idx, -X, phi, curv, surfTens, gfClamp);
			if (flags[idx + X] & MF_EMPTY) set += surfTensHelper(idx, +X, phi, curv, surfTens, gfClamp);
			if (flags[idx - Y] & MF_EMPTY) set += surfTensHelper(idx, -Y, phi, curv, surfTens, gfClamp);
			if (flags[idx + Y] & MF_EMPTY) set += surfTensHelper(idx, +Y, phi, curv, surfTens, gfClamp);
			if (d.is3d) {
				if (flags[idx - Z] & MF_EMPTY) set += surfTensHelper(idx, -Z, phi, curv, surfTens, gfClamp);
				if (flags[idx + Z] & MF_EMPTY) set += surfTensHelper(idx, +Z, phi, curv, surfTens, gfClamp);
			}
		}
		if (pcc) set += pcc[idx];
		mysum += (double)set;
		mycnt += 1.0;
		rhs[idx] = set;
	}
	mysum = block_sum(mysum);
	__syncthreads();
	mycnt = block_sum(mycnt);
	if (threadIdx.x == 0) {
		partials[blockIdx.x] = mysum;
		partials[MAX_BLOCKS + blockIdx.x] = mycnt;
	}
}
// second-level reduction for grids with more blocks than one finishing block can hold in `partials`
__global__ void __launch_bounds__(BLOCK) k_sum2_finish(int nb, const double* __restrict__ p0, const double* __restrict__ p1, double* __restrict__ out) {
	double a = strided_sum(p0, nb), b = strided_sum(p1, nb);
	a = block_sum(a);
	__syncthreads();
	b = block_sum(b);
	if (threadIdx.x == 0) {
		out[0] = a;
		out[1] = b;
	}
}

// ApplyGhostFluidDiagonal, plugin/pressure.cpp:136-151
__global__ void __launch_bounds__(BLOCK)
k_ghost_fluid_diag(Dim d, float* __restrict__ A0, const int32_t* __restrict__ flags, const float* __restrict__ phi, float gfClamp) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	if (!(flags[idx] & MF_FLUID)) return;
	const int64_t X = 1, Y = d.Y, Z = d.Z;
	float a = A0[idx];
	if (flags[idx - X] & MF_EMPTY) a -= ghostFluidHelper(idx, -X, phi, gfClamp);
	if (flags[idx + X] & MF_EMPTY) a -= ghostFluidHelper(idx, +X, phi, gfClamp);
	if (flags[idx - Y] & MF_EMPTY) a -= ghostFluidHelper(idx, -Y, phi, gfClamp);
	if (flags[idx + Y] & MF_EMPTY) a -= ghostFluidHelper(idx, +Y, phi, gfClamp);
	if (d.is3d) {
		if (flags[idx - Z] & MF_EMPTY) a -= ghostFluidHelper(idx, -Z, phi, gfClamp);
		if (flags[idx + Z] & MF_EMPTY) a -= ghostFluidHelper(idx, +Z, phi, gfClamp);
	}
	A0[idx] = a;
}

// knCorrectVelocity, plugin/pressure.cpp:87-109
__global__ void __launch_bounds__(BLOCK)
k_correct_velocity(Dim d, const int32_t* __restrict__ flags, float* __restrict__ vel, const float* __restrict__ p) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	const int64_t X = 1, Y = d.Y, Z = d.Z, n = d.n;
	float *vx = vel, *vy = vel + n, *vz = vel + 2 * n;
	const int f = flags[idx];
	if (f & MF_FLUID) {
		const float pc = p[idx];
		float x = vx[idx], y = vy[idx], z = d.is3d ? vz[idx] : 0.f;
		const int fxm = flags[idx - X], fym = flags[idx - Y], fzm = d.is3d ? flags[idx - Z] : 0;
		if (fxm & MF_FLUID) x -= (pc - p[idx - X]);
		if (fym & MF_FLUID) y -= (pc - p[idx - Y]);
		if (d.is3d && (fzm & MF_FLUID)) z -= (pc - p[idx - Z]);
		if (fxm & MF_EMPTY) x -= pc;
		if (fym & MF_EMPTY) y -= pc;
		if (d.is3d && (fzm & MF_EMPTY)) z -= pc;
		vx[idx] = x;
		vy[idx] = y;
		if (d.is3d) vz[idx] = z;
	} else if ((f & MF_EMPTY) && !(f & MF_OUTFLOW)) {
		if (flags[idx - X] & MF_FLUID) vx[idx] += p[idx - X]; else vx[idx] = 0.f;
		if (flags[idx - Y] & MF_FLUID) vy[idx] += p[idx - Y]; else vy[idx] = 0.f;
		if (d.is3d) {
			if (flags[idx - Z] & MF_FLUID) vz[idx] += p[idx - Z]; else vz[idx] = 0.f;
		}
	}
}

// knCorrectVelocityGhostFluid, plugin/pressure.cpp:154-187
__global__ void __launch_bounds__(BLOCK)
k_correct_velocity_gf(Dim d, float* __restrict__ vel, const int32_t* __restrict__ flags, const float* __restrict__ p,
                      const float* __restrict__ phi, float gfClamp, const float* __restrict__ curv, float surfTens) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	const int64_t X = 1, Y = d.Y, Z = d.Z, n = d.n;
	float *vx = vel, *vy = vel + n, *vz = vel + 2 * n;
	const int f = flags[idx];
	const bool fl = (f & MF_FLUID) != 0, emp = (f & MF_EMPTY) && !(f & MF_OUTFLOW);
	if (fl) {
		if (flags[idx - X] & MF_EMPTY) vx[idx] += p[idx] * ghostFluidHelper(idx, -X, phi, gfClamp);
		if (flags[idx - Y] & MF_EMPTY) vy[idx] += p[idx] * ghostFluidHelper(idx, -Y, phi, gfClamp);
		if (d.is3d && (flags[idx - Z] & MF_EMPTY)) vz[idx] += p[idx] * ghostFluidHelper(idx, -Z, phi, gfClamp);
	} else if (emp) {
		if (flags[idx - X] & MF_FLUID) vx[idx] -= p[idx - X] * ghostFluidHelper(idx - X, +X, phi, gfClamp); else vx[idx] = 0.f;
		if (flags[idx - Y] & MF_FLUID) vy[idx] -= p[idx - Y] * ghostFluidHelper(idx - Y, +Y, phi, gfClamp); else vy[idx] = 0.f;
		if (d.is3d) {
			if (flags[idx - Z] & MF_FLUID) vz[idx] -= p[idx - Z] * ghostFluidHelper(idx - Z, +Z, phi, gfClamp); else vz[idx] = 0.f;
		}
	}
	if (curv) {
		if (fl) {
			if (flags[idx - X] & MF_EMPTY) vx[idx] += surfTensHelper(idx, -X, phi, curv, surfTens, gfClamp);
			if (flags[idx - Y] & MF_EMPTY) vy[idx] += surfTensHelper(idx, -Y, phi, curv, surfTens, gfClamp);
			if (d.is3d && (flags[idx - Z] & MF_EMPTY)) vz[idx] += surfTensHelper(idx, -Z, phi, curv, surfTens, gfClamp);
		} else if (emp) {
			vx[idx] -= (flags[idx - X] & MF_FLUID) ? surfTensHelper(idx - X, +X, phi, curv, surfTens, gfClamp) : 0.f;
			vy[idx] -= (flags[idx - Y] & MF_FLUID) ? surfTensHelper(idx - Y, +Y, phi, curv, surfTens, gfClamp) : 0.f;
			if (d.is3d) vz[idx] -= (flags[idx - Z] & MF_FLUID) ? surfTensHelper(idx - Z, +Z, phi, curv, surfTens, gfClamp) : 0.f;
		}
	}
}

// knReplaceClampedGhostFluidVels, plugin/pressure.cpp:198-214.  Writes touch empty cells' components, reads
// touch fluid cells' components of the same grid: disjoint, so in-place is race free.
__global__ void __launch_bounds__(BLOCK)
k_replace_clamped_gf(Dim d, float* __restrict__ vel, const int32_t* __restrict__ flags, const float* __restrict__ phi, float gfClamp) {
	CELL_IJK(d)
	if (!INTERIOR(d)) return;
	if (!(flags[idx] & MF_EMPTY)) return;
	const int64_t X = 1, Y = d.Y, Z = d.Z, n = d.n;
	float *vx = vel, *vy = vel + n, *vz = vel + 2 * n;
	if ((flags[idx - X] & MF_FLUID) && ghostFluidWasClamped(idx - X, +X, phi, gfClamp)) vx[idx] = vx[idx - X];
	if ((flags[idx - Y] & MF_FLUID) && ghostFluidWasClamped(idx - Y, +Y, phi, gfClamp)) vy[idx] = vy[idx - Y];
	if (d.is3d && (flags[idx - Z] & MF_FLUID) && ghostFluidWasClamped(idx - Z, +Z, phi, gfClamp)) vz[idx] = vz[idx - Z];
	if ((flags[idx + X] & MF_FLUID) && ghostFluidWasClamped(idx + X, -X, phi, gfClamp)) vx[idx] = vx[idx + X];
	if ((flags[idx + Y] & MF_FLUID) && ghostFluidWasClamped(idx + Y, -Y, phi, gfClamp)) vy[idx] = vy[idx + Y];
	if (d.is3d && (flags[idx + Z] & MF_FLUID) && ghostFluidWasClamped(idx + Z, -Z, phi, gfClamp)) vz[idx] = vz[idx + Z];
}

// fixPressure, plugin/pressure.cpp:226-246 (a handful of scalar updates: one thread)
__global__ void k_fix_pressure(Dim d, int64_t p, float value, float* rhs, float* A0, float* Ai, float* Aj, float* Ak) {
	const int64_t X = 1, Y = d.Y, Z = d.Z;
	rhs[p + X] -= Ai[p] * value;
	rhs[p + Y] -= Aj[p] * value;
	rhs[p - X] -= Ai[p - X] * value;
	rhs[p - Y] -= Aj[p - Y] * value;
	if (d.is3d) {
		rhs[p + Z] -= Ak[p] * value;
		rhs[p - Z] -= Ak[p - Z] * value;
	}
	rhs[p] = value;
	A0[p] = 1.f;
	Ai[p] = Aj[p] = Ak[p] = 0.f;
	Ai[p - X] = 0.f;
	Aj[p - Y] = 0.f;
	if (d.is3d) Ak[p - Z] = 0.f;
}

// =========================================================================================================
// PCG scalar kernels (one block) -- scalars never leave the device inside an iteration
// =========================================================================================================
__global__ void __launch_bounds__(BLOCK) k_cg_begin(CgScalars* sc, int nb, const double* __restrict__ partials, float accuracy, int useL2) {
	double acc = strided_sum(partials, nb);
	acc = block_sum(acc);
	if (threadIdx.x == 0) {
		sc->sigma = (float)acc;  // mSigma = GridDotProduct(mTmp, mResidual), conjugategrad.cpp:234
		sc->alpha = sc->nalpha = sc->beta = 0.f;
		sc->resNorm = 1e20f;
		sc->accuracy = accuracy;
		sc->iterations = 0;
		sc->done = 0;
		sc->diverged = 0;
		sc->useL2 = useL2;
	}
}
// alpha = sigma / dp, conjugategrad.cpp:250-252
__global__ void __launch_bounds__(BLOCK) k_cg_alpha(CgScalars* sc, int nb, const double* __restrict__ partials) {
	if (sc->done) {
		if (threadIdx.x == 0) sc->xpending = 0;
		return;
	}
	if (sc->diverged) {
		// the iteration that diverged has finished its search update (the reference throws after it): stop everything queued
		// behind it.  (This iteration's ApplyMatrix has already run; it only wrote tmp.)
		if (threadIdx.x == 0) {
			sc->done = 1;
			sc->xpending = 0;
		}
		return;
	}
	double acc = strided_sum(partials, nb);
	acc = block_sum(acc);
	if (threadIdx.x == 0) {
		const float dp = (float)acc;
		float alpha = 0.f;
		if (fabs((double)dp) > 0.) alpha = sc->sigma / dp;
		sc->dp = dp;
		sc->alpha = alpha;
		sc->nalpha = -alpha;
		sc->iterations++;
		sc->xpending = 1;
	}
}
// ---- the two vector passes of an iteration, one body each: the kernels below differ in where their scalars come from and in the
// template flags.  VEC: quads (16-byte aligned views) with the n & 3 cells behind the last quad done by block 0, or cell by cell.
// what rides on the residual pass of k_cg_axpy2: dst += alpha * search (conjugategrad.cpp:254)
struct NoRider {
	__device__ __forceinline__ void quad(int64_t) const {}
	__device__ __forceinline__ void cell(int64_t) const {}
};
struct XUpdateRider {
	float* __restrict__ dst;
	const float* __restrict__ search;
	float alpha;
	__device__ __forceinline__ void quad(int64_t q) const { ((float4*)dst)[q] = axpy4(((float4*)dst)[q], alpha, ((const float4*)search)[q]); }
	__device__ __forceinline__ void cell(int64_t i) const { dst[i] = dst[i] + alpha * search[i]; }
};
// residual += nalpha * tmp (conjugategrad.cpp:265) ; COPY_TMP (PC_NONE): tmp = residual ; per block the min / max of the new residual
// -> fpart, or (l2) its sum of squares -> dpart (:268-272).  nt: tmp is read non-temporally (alone: 64.4 vs 63.7 ms per step).
// EDOT (liquid scenes): the MIC sweeps leave bundles of rows without fluid out, so tmp is in those cells what it is here and their share
// of dot(M^-1 r, r) = sum tmp * r_new can be formed in this pass, which streams both anyway (sx % 4 == 0, so a quad lies in one row);
// the shares go to epart[block] and are appended to the sweep's partials (whose entries for those bundles are 0) -- whether or not the
// premise of the skip map holds.  A kernel of its own for them cost 33 us per iteration in the 379 x 356 x 124 dam break.  While the
// premise holds (skip.active()), residual and tmp are zero in what the map leaves out and stay so: those quads are neither read nor
// written, they enter the min / max as the zeros they are and add nothing to the sums.
template <bool COPY_TMP, bool EDOT, bool VEC, class Rider = NoRider>
__device__ __forceinline__ void residual_pass(int64_t n, float nalpha, bool l2, float* __restrict__ residual, float* __restrict__ tmp, bool nt,
                                              float* __restrict__ fpart, double* __restrict__ dpart, const SkipMap& skip = SkipMap{}, int sx = 0,
                                              int sy = 0, double* __restrict__ epart = nullptr, const Rider& rider = Rider{}) {
	const bool zero_outside = EDOT && skip.active();
	const SkipMap::XRange xr = EDOT ? skip.range(sx) : SkipMap::XRange{0, 0};
	float lo = FLT_MAX, hi = -FLT_MAX;
	double ss = 0.0, es = 0.0;
	auto cell = [&](int64_t i) {
		rider.cell(i);
		const float r = residual[i] + nalpha * tmp[i];
		residual[i] = r;
		if (COPY_TMP) tmp[i] = r;
		if (l2) ss += (double)r * (double)r;
		lo = fminf(lo, r);
		hi = fmaxf(hi, r);
	};
	if (VEC) {
		const int64_t n4 = n >> 2;
		for (int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x; q < n4; q += (int64_t)gridDim.x * BLOCK) {
			bool in_empty = false;
			if (EDOT) {
				int j, k, x;
				quad_cell(q, sx, sy, j, k, x);
				in_empty = skip.empty_bundle(j, k);
				if (zero_outside && (in_empty || xr.outside(x))) {
					lo = fminf(lo, 0.f);
					hi = fmaxf(hi, 0.f);
					continue;
				}
			}
			rider.quad(q);
			const float4 r0 = ((float4*)residual)[q], t = ld4(tmp + 4 * q, nt);
			const float4 r = axpy4(r0, nalpha, t);
			((float4*)residual)[q] = r;
			if (COPY_TMP) ((float4*)tmp)[q] = r;
			if (EDOT && in_empty) es = dot4(es, t, r);
			if (l2) ss = sumsq4(ss, r);
			else {
				lo = min4(lo, r);
				hi = max4(hi, r);
			}
		}
		if (blockIdx.x == 0 && threadIdx.x < (n & 3)) cell((n4 << 2) + threadIdx.x);
	} else {
		for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) cell(i);
	}
	if (l2) {
		ss = block_sum(ss);
		if (threadIdx.x == 0) dpart[blockIdx.x] = ss;
	} else {
		block_minmax(lo, hi);
		if (threadIdx.x == 0) {
			fpart[2 * blockIdx.x] = lo;
			fpart[2 * blockIdx.x + 1] = hi;
		}
	}
	if (EDOT) {
		__syncthreads();
		es = block_sum(es);
		if (threadIdx.x == 0) epart[blockIdx.x] = es;
	}
}
// dst += alpha * search (conjugategrad.cpp:254) and, with upd, search = tmp + beta * search (:283) -- `search` is read once for both.
// nt: the pressure is touched here and nowhere else in an iteration, tmp for the last time before ApplyMatrix overwrites it: non-temporal,
// so that 128 MB per 256^3 iteration do not displace what the sweeps and the stencil re-read (63.1 vs 63.7 ms per step of tools/micro/ntv_bench.py).
// SKIP (liquid scenes): dst, search and tmp are zero in what the map leaves out and stay zero
template <bool SKIP, bool VEC>
__device__ __forceinline__ void search_pass(int64_t n, float alpha, float beta, bool upd, float* __restrict__ dst, float* __restrict__ search,
                                            const float* __restrict__ tmp, bool nt, const SkipMap& skip = SkipMap{}, int sx = 0, int sy = 0) {
	auto cell = [&](int64_t i) {
		const float s = search[i];
		dst[i] = dst[i] + alpha * s;
		if (upd) search[i] = tmp[i] + beta * s;
	};
	if (VEC) {
		const SkipMap::XRange xr = SKIP ? skip.range(sx) : SkipMap::XRange{0, 0};
		const bool zero_outside = SKIP && skip.active();
		const int64_t n4 = n >> 2;
		for (int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x; q < n4; q += (int64_t)gridDim.x * BLOCK) {
			if (SKIP && zero_outside) {
				int j, k, x;
				quad_cell(q, sx, sy, j, k, x);
				if (skip.empty_bundle(j, k) || xr.outside(x)) continue;
			}
			const float4 s = ld4(search + 4 * q, nt);
			st4(dst + 4 * q, axpy4(ld4(dst + 4 * q, nt), alpha, s), nt);
			if (upd) st4(search + 4 * q, axpy4(ld4(tmp + 4 * q, nt), beta, s), nt);
		}
		if (blockIdx.x == 0 && threadIdx.x < (n & 3)) cell((n4 << 2) + threadIdx.x);
	} else {
		for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) cell(i);
	}
}

// the residual update of mf_cg_solve: k_cg_axpy2 without the dst update, which is left to k_cg_update_search_x (one pass over `search`
// less per iteration)
// (Folding this pass into the loader waves of the forward MIC sweep -- they read residual and tmp anyway -- was built and measured:
// bit-exact, the 30 us of this kernel go away and the sweep gets 21 us slower (its middle third already streams ~4 TB/s): 75.5 ms per
// 256^3 step either way.  Not kept.)
template <bool COPY_TMP, bool EDOT = false>
__global__ void __launch_bounds__(BLOCK)
k_cg_axpy_r(int64_t n, const CgScalars* __restrict__ sc, float* __restrict__ residual, float* __restrict__ tmp, float* __restrict__ fpart,
            double* __restrict__ dpart, SkipMap skip = SkipMap{}, int sx = 0, int sy = 0, double* __restrict__ epart = nullptr, int nt = 0) {
	if (sc->done) return;
	residual_pass<COPY_TMP, EDOT, true>(n, sc->nalpha, sc->useL2 != 0, residual, tmp, nt != 0, fpart, dpart, skip, sx, sy, epart);
}
// dst += alpha*search ; residual += (-alpha)*tmp ; partial min/max (or sum of squares) of the new residual.
// conjugategrad.cpp:254-255, 265, 268-272
__global__ void __launch_bounds__(BLOCK)
k_cg_axpy2(int64_t n, const CgScalars* __restrict__ sc, float* __restrict__ dst, const float* __restrict__ search,
           float* __restrict__ residual, float* __restrict__ tmp, float* __restrict__ fpart, double* __restrict__ dpart) {
	if (sc->done) return;
	residual_pass<false, false, true>(n, sc->nalpha, sc->useL2 != 0, residual, tmp, false, fpart, dpart, SkipMap{}, 0, 0, nullptr,
	                                  XUpdateRider{dst, search, sc->alpha});
}
// sigmaNew partials: GridDotProduct(tmp, residual), conjugategrad.cpp:279
__global__ void __launch_bounds__(BLOCK)
k_cg_dot(int64_t n, const CgScalars* __restrict__ sc, const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ partials) {
	if (sc->done) return;
	double acc = 0.0;
	const int64_t n4 = n >> 2;
	for (int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x; q < n4; q += (int64_t)gridDim.x * BLOCK)
		acc = dot4(acc, ((const float4*)a)[q], ((const float4*)b)[q]);
	if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
		const int64_t i = (n4 << 2) + threadIdx.x;
		const float p = a[i] * b[i];
		acc += (double)p;
	}
	acc = block_sum(acc);
	if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}
// residual norm, convergence test, beta.  conjugategrad.cpp:268-295
__global__ void __launch_bounds__(BLOCK)
k_cg_beta(CgScalars* sc, int nbr, const float* __restrict__ fpart, const double* __restrict__ dpart_res, int nbd,
          const double* __restrict__ dpart_dot) {
	if (sc->done) return;
	float lo = FLT_MAX, hi = -FLT_MAX;
	double ss = 0.0, dd = 0.0;
	const bool l2 = sc->useL2 != 0;
	for (int i = threadIdx.x; i < nbr; i += blockDim.x) {
		if (l2)
			ss += dpart_res[i];
		else {
			lo = fminf(lo, fpart[2 * i]);
			hi = fmaxf(hi, fpart[2 * i + 1]);
		}
	}
	dd = strided_sum(dpart_dot, nbd);
	block_minmax(lo, hi);
	__syncthreads();
	ss = block_sum(ss);
	__syncthreads();
	dd = block_sum(dd);
	if (threadIdx.x == 0) cg_beta_step(sc, l2, lo, hi, ss, dd);
}
// the search update of mf_cg_solve: this iteration's dst += alpha*search is still to be done (xpending), the search direction is
// renewed unless the iteration has converged
template <bool SKIP>
__global__ void __launch_bounds__(BLOCK)
k_cg_update_search_x(int64_t n, const CgScalars* __restrict__ sc, float* __restrict__ dst, float* __restrict__ search, const float* __restrict__ tmp,
                     SkipMap skip = SkipMap{}, int sx = 0, int sy = 0, int nt = 0) {
	if (!sc->xpending) return;
	search_pass<SKIP, true>(n, sc->alpha, sc->beta, !sc->done, dst, search, tmp, nt != 0, skip, sx, sy);
}
// the same for views that do not start on a 16-byte boundary
__global__ void __launch_bounds__(BLOCK)
k_cg_update_search_x_scalar(int64_t n, const CgScalars* __restrict__ sc, float* __restrict__ dst, float* __restrict__ search, const float* __restrict__ tmp) {
	if (!sc->xpending) return;
	search_pass<false, false>(n, sc->alpha, sc->beta, !sc->done, dst, search, tmp, false);
}
// z-slab PCG scalar steps on the gathered per-rank reductions (common.h: slab_alpha, slab_beta_stop), on a CgScalars block: `done`
// mirrors the stop state, `xpending` says that this iteration's x += alpha * search is still to be done by the search update
__global__ void k_slab_alpha_x(const double* __restrict__ g, int world, CgScalars* __restrict__ sc, const int32_t* __restrict__ state) {
	if (state && state[0]) {
		sc->alpha = 0.f;
		sc->nalpha = -0.f;
		sc->xpending = 0;
		sc->done = 1;
		return;
	}
	const float a = slab_alpha(g, world, sc->sigma);
	sc->alpha = a;
	sc->nalpha = -a;
	sc->xpending = 1;
	sc->done = 0;
	sc->sigmaPrev = sc->sigma;
}
// k_slab_alpha_x + the residual update (min / max partials) in one launch: every block forms alpha from the gathered rows itself (the
// same bits everywhere), block 0 publishes the scalars for the kernels behind it.  Nothing this kernel writes is read by another block
// of it (sigma and the stop state are written by the search update's kernel only).
__global__ void __launch_bounds__(BLOCK)
k_slab_axpy_r(int64_t n, const double* __restrict__ g, int world, CgScalars* __restrict__ sc, const int32_t* __restrict__ state,
              float* __restrict__ residual, const float* __restrict__ tmp, float* __restrict__ fpart, int nt) {
	const bool stopped = state[0] != 0;
	const float a = stopped ? 0.f : slab_alpha(g, world, sc->sigma);
	const float nalpha = -a;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		sc->alpha = a;
		sc->nalpha = nalpha;
		sc->xpending = stopped ? 0 : 1;
		sc->done = stopped ? 1 : 0;
		if (!stopped) sc->sigmaPrev = sc->sigma;
	}
	if (stopped) return;
	residual_pass<false, false, true>(n, nalpha, false, residual, (float*)tmp, nt != 0, fpart, nullptr);
}
// the residual update for views that do not start on a 16-byte boundary, behind k_slab_alpha_x: nothing once stopped (`done`), so that the
// residual keeps its bits -- r + (-0) * tmp would turn a -0 into +0, and into NaN where tmp has overflowed
__global__ void __launch_bounds__(BLOCK)
k_slab_axpy_r_scalar(int64_t n, const CgScalars* __restrict__ sc, float* __restrict__ residual, const float* __restrict__ tmp, float* __restrict__ fpart) {
	if (sc->done) return;
	residual_pass<false, false, false>(n, sc->nalpha, false, residual, (float*)tmp, false, fpart, nullptr);
}
__global__ void k_slab_beta_x(const double* __restrict__ g, int world, CgScalars* __restrict__ sc, float accuracy, int iter, int32_t* __restrict__ state) {
	if (state && state[0]) return;
	const SlabBeta b = slab_beta_stop(g, world, sc->sigma, accuracy);
	sc->resNorm = b.resNorm;
	sc->beta = b.beta;
	sc->sigma = b.sigmaNew;
	if (state && b.stop) {
		state[0] = b.stop;
		state[1] = iter;
		sc->done = 1;
	}
}
// k_slab_beta_x + the search update in one launch, the same way: every block forms beta and the stopping test from the gathered rows,
// block 0 publishes them (sigma, the stop state) -- the other blocks read sigmaPrev / xpending / alpha, which the residual update's
// kernel wrote
__global__ void __launch_bounds__(BLOCK)
k_slab_update_search_x(int64_t n, const double* __restrict__ g, int world, CgScalars* __restrict__ sc, float accuracy, int iter,
                       int32_t* __restrict__ state, float* __restrict__ dst, float* __restrict__ search, const float* __restrict__ tmp, int nt) {
	if (!sc->xpending) return;          // stopped before this iteration
	const SlabBeta b = slab_beta_stop(g, world, sc->sigmaPrev, accuracy);
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		sc->resNorm = b.resNorm;
		sc->beta = b.beta;
		sc->sigma = b.sigmaNew;
		if (b.stop) {
			state[0] = b.stop;
			state[1] = iter;
			sc->done = 1;
		}
	}
	search_pass<false, true>(n, sc->alpha, b.beta, !b.stop, dst, search, tmp, nt != 0);
}

// cgSolveDiffusion matrix set-up, conjugategrad.cpp:364-375
__global__ void __launch_bounds__(BLOCK)
k_diffusion_matrix(int64_t n, const int32_t* __restrict__ flags, float* __restrict__ A0, float* __restrict__ Ai, float* __restrict__ Aj,
                   float* __restrict__ Ak, float alpha) {
	const int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (idx >= n) return;
	if (flags[idx] & MF_OBSTACLE) {
		Ai[idx] = Aj[idx] = Ak[idx] = 0.f;
		A0[idx] = 1.f;
	} else {
		Ai[idx] *= alpha;
		Aj[idx] *= alpha;
		Ak[idx] *= alpha;
		A0[idx] = A0[idx] * alpha + 1.f;      // two roundings (-ffp-contract=off), as "A0 *= alpha; A0 += 1." in the reference
	}
}

// the system of mf_cg_solve with its rows padded from sx to px cells (pad cells: obstacle, zero coefficients, zero rhs), plus the caller's
// tmp (pad cells 0), and back
__global__ void __launch_bounds__(BLOCK)
k_pad_system(int sx, int px, int64_t np_, const int32_t* __restrict__ flags, const float* __restrict__ rhs, const float* __restrict__ tmp,
             const float* __restrict__ A0, const float* __restrict__ Ai, const float* __restrict__ Aj, const float* __restrict__ Ak,
             int32_t* __restrict__ pf, float* __restrict__ pr, float* __restrict__ pt, float* __restrict__ p0, float* __restrict__ pi,
             float* __restrict__ pj, float* __restrict__ pk) {
	for (int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x; q < np_; q += (int64_t)gridDim.x * BLOCK) {
		const int64_t row = q / px;
		const int i = (int)(q - row * px);
		const bool in = i < sx;
		const int64_t s = row * sx + i;
		pf[q] = in ? flags[s] : MF_OBSTACLE;
		pr[q] = in ? rhs[s] : 0.f;
		pt[q] = in ? tmp[s] : 0.f;
		p0[q] = in ? A0[s] : 0.f;
		pi[q] = in ? Ai[s] : 0.f;
		pj[q] = in ? Aj[s] : 0.f;
		pk[q] = in ? Ak[s] : 0.f;
	}
}
__global__ void __launch_bounds__(BLOCK)
k_unpad(int sx, int px, int64_t n, const float* __restrict__ padded, float* __restrict__ out) {
	for (int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x; q < n; q += (int64_t)gridDim.x * BLOCK) {
		const int64_t row = q / sx;
		out[q] = padded[row * px + (q - row * sx)];
	}
}

// the padded copy of mf_cg_solve's system, per device (solves on one device are ordered on one stream): 11 slices of one arena block
// -- flags, dst, rhs, residual, search, tmp, A0, Ai, Aj, Ak, Aprecond -- of this solve's padded cell count each, cut per solve.  The
// block follows the growth rule of every arena (arena_reserve: to max(2 * cap, need) after a device synchronise, never shrinks).
static Arena g_pad[MAX_DEVICES];

// Liquid scenes: most 8 x 8 bundles of rows hold no fluid cell (benchmark_dam.py: 6 % of the cells are fluid).  MakeRhs leaves rhs zero
// outside the fluid and the work grids are fresh zero grids, so every PCG vector is zero in those bundles and stays zero (ApplyMatrix copies
// src, the sweeps leave them out, the vector updates combine zeros) -- the kernels of an iteration then skip them altogether.  This kernel
// is what establishes the premise, on the device, once per solve: bad[0] counts the quads of empty bundles in which rhs or tmp is not +0.
// x-range of the packed system (bytes of k_mic_pack / k_setup_fused; sx % 8 == 0): xr[0] = first cell with a non-zero byte, xr[1] = one
// past the last one, plus one (a set "Ai is -1" bit couples the cell behind it).  Cells outside are non-fluid cells without couplings.
__global__ void __launch_bounds__(BLOCK)
k_pack_xrange(int64_t n, int sx, const unsigned char* __restrict__ pack, int* __restrict__ xr) {
	int lo = 0x7fffffff, hi = 0;
	const int64_t n8 = n >> 3;
	for (int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x; q < n8; q += (int64_t)gridDim.x * BLOCK) {
		const unsigned long long w = ((const unsigned long long*)pack)[q];
		if (w == 0ull) continue;
		const int x0 = (int)((8 * q) % sx);
		const int a = x0 + (__ffsll((long long)w) - 1) / 8, b = x0 + (63 - __clzll((long long)w)) / 8 + 2;
		lo = a < lo ? a : lo;
		hi = b > hi ? b : hi;
	}
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) {
		const int l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
		lo = l2 < lo ? l2 : lo;
		hi = h2 > hi ? h2 : hi;
	}
	if ((threadIdx.x & 63) == 0 && hi > 0) {
		atomicMin(&xr[0], lo);
		atomicMax(&xr[1], hi);
	}
}
__global__ void __launch_bounds__(BLOCK)
k_cg_outside_zero(int64_t n, int sx, int sy, SkipMap skip, const float* __restrict__ rhs, const float* __restrict__ tmp,
                  const float* __restrict__ search, int* __restrict__ bad) {      // (bad: what skip.outside_bad points to, still to be written)
	const int64_t n4 = n >> 2;
	int found = 0;
	const SkipMap::XRange xr = skip.range(sx);
	for (int64_t q = blockIdx.x * (int64_t)BLOCK + threadIdx.x; q < n4; q += (int64_t)gridDim.x * BLOCK) {
		int j, k, x;
		quad_cell(q, sx, sy, j, k, x);
		if (!skip.empty_bundle(j, k) && !xr.outside(x)) continue;
		const uint4 a = ((const uint4*)rhs)[q], b = ((const uint4*)tmp)[q], c = ((const uint4*)search)[q];
		if ((a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w | c.x | c.y | c.z | c.w) != 0u) found = 1;
	}
	if (__any(found) && (threadIdx.x & 63) == 0) atomicAdd(bad, 1);
}
// ---- matrix-free set-up of a plain MakeLaplaceMatrix system (no fractions, no ghost fluid, no optional rhs terms): ONE pass over
// flags and vel writes rhs (MakeRhs, pressure.cpp:32-84), the packed byte of every cell -- fluid bit, "Ai / Aj / Ak is -1" bits and the
// integer diagonal in bits 4-7 (MakeLaplaceMatrix, conjugategrad.h:154-187; k_mic_pack's layout) -- and clears the empty-bundle entry
// of every 8 x 8 bundle of rows that holds a fluid cell.  The float arrays A0 / Ai / Aj / Ak never exist.  A thread owns 4 cells.
__global__ void __launch_bounds__(BLOCK)
k_setup_fused(Dim d, const int32_t* __restrict__ flags, const float* __restrict__ vel, float* __restrict__ rhs, unsigned char* __restrict__ pack,
              int* __restrict__ bempty, int nbj) {
	const int qx = d.sx >> 2;
	const int64_t T = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
	if (T >= (int64_t)qx * d.sy * d.sz) return;
	const int qi = (int)(T % qx);
	const int64_t rg = T / qx;
	const int j = (int)(rg % d.sy), k = (int)(rg / d.sy), i0 = 4 * qi;
	const int64_t Y = d.Y, Z = d.Z, n = d.n;
	const int64_t idx = i0 + Y * j + Z * k;
	const int4 f4 = *(const int4*)(flags + idx);
	const int f[4] = {f4.x, f4.y, f4.z, f4.w};
	float r[4] = {0.f, 0.f, 0.f, 0.f};
	unsigned bytes = 0;
	const bool row_in = j >= 1 && j <= d.sy - 2 && k >= 1 && k <= d.sz - 2;
	if (row_in) {
		const int4 ym4 = *(const int4*)(flags + idx - Y), yp4 = *(const int4*)(flags + idx + Y);
		const int4 zm4 = *(const int4*)(flags + idx - Z), zp4 = *(const int4*)(flags + idx + Z);
		const int ym[4] = {ym4.x, ym4.y, ym4.z, ym4.w}, yp[4] = {yp4.x, yp4.y, yp4.z, yp4.w};
		const int zm[4] = {zm4.x, zm4.y, zm4.z, zm4.w}, zp[4] = {zp4.x, zp4.y, zp4.z, zp4.w};
		const int fxm = i0 > 0 ? flags[idx - 1] : MF_OBSTACLE, fxp = i0 + 4 < d.sx ? flags[idx + 4] : MF_OBSTACLE;
		const float *vx = vel, *vy = vel + n, *vz = vel + 2 * n;
		const float4 ux4 = *(const float4*)(vx + idx), uy4 = *(const float4*)(vy + idx), uyp4 = *(const float4*)(vy + idx + Y);
		const float4 uz4 = *(const float4*)(vz + idx), uzp4 = *(const float4*)(vz + idx + Z);
		const float uxp = i0 + 4 < d.sx ? vx[idx + 4] : 0.f;
		const float ux[5] = {ux4.x, ux4.y, ux4.z, ux4.w, uxp};
		const float uy[4] = {uy4.x, uy4.y, uy4.z, uy4.w}, uyp[4] = {uyp4.x, uyp4.y, uyp4.z, uyp4.w};
		const float uz[4] = {uz4.x, uz4.y, uz4.z, uz4.w}, uzp[4] = {uzp4.x, uzp4.y, uzp4.z, uzp4.w};
#pragma unroll
		for (int c = 0; c < 4; c++) {
			const int i = i0 + c;
			const bool fl = (f[c] & MF_FLUID) != 0;
			unsigned b = pk_make(fl, false, false, false, 0u);
			if (fl && i >= 1 && i <= d.sx - 2) {
				const int xm = c > 0 ? f[c - 1] : fxm, xp = c < 3 ? f[c + 1] : fxp;
				const unsigned a0 = (unsigned)!(xm & MF_OBSTACLE) + (unsigned)!(xp & MF_OBSTACLE) + (unsigned)!(ym[c] & MF_OBSTACLE) +
				                    (unsigned)!(yp[c] & MF_OBSTACLE) + (unsigned)!(zm[c] & MF_OBSTACLE) + (unsigned)!(zp[c] & MF_OBSTACLE);
				b = pk_make(true, xp & MF_FLUID, yp[c] & MF_FLUID, zp[c] & MF_FLUID, a0);
				float set = ux[c] - ux[c + 1] + uy[c] - uyp[c];
				set += uz[c] - uzp[c];
				r[c] = set;
			}
			bytes |= b << (8 * c);
		}
	} else {
#pragma unroll
		for (int c = 0; c < 4; c++) bytes |= pk_make(f[c] & MF_FLUID, false, false, false, 0u) << (8 * c);
	}
	*(float4*)(rhs + idx) = make_float4(r[0], r[1], r[2], r[3]);
	*(unsigned*)(pack + idx) = bytes;
	if (bytes & (PK_FLUID * PK_WORD)) bempty[(k >> 3) * nbj + (j >> 3)] = 0;
}

// What the iterations of one PCG solve run, decided once before the first of them (pcg_setup); the iteration loop reads nothing else.
// Liquid scenes: am.skip is what the kernels of an iteration leave out (pressure.h: SkipMap); where the sweep's workgroups draw several bundles each, be_map is the same map
// for the sweep: the dot shares of its empty bundles then ride on the residual update (k_cg_axpy_r<.., EDOT>), behind its partials.
struct PcgPlan {
	AmOpts am;                    // ApplyMatrix: packed bytes, skip map, x-range, non-temporal policy (also that of the vector kernels)
	const int* be_map = nullptr;
	MicSweep sweep;               // the x-range trim of the MIC sweeps
};
// The set-up after doInit: packed bytes, empty-bundle maps, x-range verdict (one read-back), non-temporal policy -> *p and
// g_last_shortcut.  free_pack (mf_solve_pressure_fused): the system exists as packed bytes only.
static int pcg_setup(const Dim& d, const int32_t* flags, const float* rhs, const float* search, const float* tmp, const float* A0, const float* Ai,
                     const float* Aj, const float* Ak, const float* Aprecond, int pc, const unsigned char* free_pack, Workspace* ws, hipStream_t st,
                     PcgPlan* p) {
	const int sx = d.sx, sy = d.sy;
	const int64_t n = d.n;
	const int nbs = blocks_for(n >> 2, BLOCK, 2048);
	// ApplyMatrix reads the same packed coefficient bytes as the MIC sweeps when mf_mic_init found the matrix packable
	if (free_pack) {
		p->am.pack = free_pack;
		p->am.a0_packed = true;
	} else if (pc == MF_PC_MICP) {
		MF_TRY(mic_pack_query(d, flags, A0, Ai, Aj, Ak, &p->am.pack, &p->am.a0_packed, st));
	}
	bool several = false;
	if (pc == MF_PC_MICP && (sx % 4) == 0) MF_TRY(mic_empty_map(d, flags, Aprecond, Aj, Ak, &p->am.skip.bempty, &p->am.skip.nbj, &several, st));
	if (several) p->be_map = p->am.skip.bempty;
	g_last_shortcut[0] = g_last_shortcut[1] = g_last_shortcut[2] = 0;
	p->am.nt = (!p->am.skip.on() && n > PCG_NT_CELLS) ? 1 : 0;
	if (p->am.skip.on()) {
		// (n % 4 == 0 here: sx % 4 == 0.)  residual = rhs and dst = 0 were set by doInit; tmp and search are the caller's
		int* p_bad = (int*)((char*)ws->scalars + WS_PCG_FLAGS);
		int* p_xr = p_bad + 1;
		const bool ranged = p->am.pack != nullptr && (sx % 8) == 0;
		p->am.skip.outside_bad = p_bad;
		if (ranged) p->am.skip.xr = p_xr;
		const int init3[3] = {0, 0x7fffffff, 0};
		MF_HIP(hipMemcpyAsync(p_bad, init3, sizeof init3, hipMemcpyHostToDevice, st));
		if (ranged) hipLaunchKernelGGL(k_pack_xrange, dim3(blocks_for(n >> 3, BLOCK, 2048)), dim3(BLOCK), 0, st, n, sx, p->am.pack, p_xr);
		hipLaunchKernelGGL(k_cg_outside_zero, dim3(nbs), dim3(BLOCK), 0, st, n, sx, sy, p->am.skip, rhs, tmp, search, p_bad);
		MF_LAUNCH_CHECK();
		if (ranged) {
			// the sweeps keep to the x-range of the fluid, if the host may know that everything outside is +0
			int h3[3] = {1, 0, 0};
			MF_HIP(hipMemcpyAsync(h3, p_bad, sizeof h3, hipMemcpyDeviceToHost, st));
			MF_HIP(hipStreamSynchronize(st));
			const SkipMap::XRange xr = SkipMap::rounded(h3[1], h3[2]);
			int c0 = xr.lo / 8, c1 = xr.hi / 8;
			if (c1 > sx / 8) c1 = sx / 8;
			if (h3[0] == 0 && h3[2] > 0 && c1 > c0) {
				p->sweep.trim_xoff = 8 * c0;
				p->sweep.trim_chunks = c1 - c0;
				g_last_shortcut[0] = 1;
				if (c1 - c0 < sx / 8) {
					g_last_shortcut[1] = 8 * c0;
					g_last_shortcut[2] = 8 * (c1 - c0);
				}
			}
		}
	}
	return 0;
}
// doInit + iterate loop of GridCg (conjugategrad.cpp:210-307).  free_pack (mf_solve_pressure_fused): the system exists as packed bytes
// only -- A0 / Ai / Aj / Ak are null, the MIC factor is already in Aprecond and the system is registered with the sweeps
static int cg_solve_core(const Dim& d, const int32_t* flags, float* dst, const float* rhs, float* residual, float* search, float* tmp,
                         const float* A0, const float* Ai, const float* Aj, const float* Ak, float* Aprecond, int pc, float accuracy,
                         int maxIter, int useL2Norm, float* out_host, void* stream, const unsigned char* free_pack, const PcExternal* ext = nullptr) {
	const int sx = d.sx, sy = d.sy, sz = d.sz;
	const int64_t n = d.n;
	hipStream_t st = (hipStream_t)stream;
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	CgScalars* sc = (CgScalars*)ws->scalars;
	double* p_dot = ws->partials;                   // apply-matrix / sigma dot partials
	double* p_res = ws->partials + MAX_BLOCKS;      // sum-of-squares partials of the residual
	double* p_sig = ws->partials + 2 * MAX_BLOCKS;  // dot(tmp, residual) partials
	float* p_mm = ws->fpartials;
	const int nbs = blocks_for(n >> 2, BLOCK, 2048);

	// ---- doInit, conjugategrad.cpp:210-235 ----
	MF_HIP(hipMemsetAsync(dst, 0, sizeof(float) * n, st));
	MF_HIP(hipMemcpyAsync(residual, rhs, sizeof(float) * n, hipMemcpyDeviceToDevice, st));
	if (pc == MF_PC_MICP) {
		if (!free_pack) MF_TRY(mf_mic_init(sx, sy, sz, flags, Aprecond, A0, Ai, Aj, Ak, stream));
		MF_TRY(mf_mic_apply(sx, sy, sz, flags, tmp, residual, Aprecond, Ai, Aj, Ak, stream));
	} else if (ext) {
		// PC_MGP: InitPreconditionMultigrid + ApplyPreconditionMultigrid, conjugategrad.cpp:229-231
		MF_TRY(ext->init(ext->ctx, A0, Ai, Aj, Ak, accuracy, st));
		MF_TRY(ext->apply(ext->ctx, tmp, residual, st));
	} else {
		MF_HIP(hipMemcpyAsync(tmp, residual, sizeof(float) * n, hipMemcpyDeviceToDevice, st));
	}
	MF_HIP(hipMemcpyAsync(search, tmp, sizeof(float) * n, hipMemcpyDeviceToDevice, st));
	MF_HIP(hipMemsetAsync(sc, 0, sizeof(CgScalars), st));
	hipLaunchKernelGGL(k_cg_dot, dim3(nbs), dim3(BLOCK), 0, st, n, sc, tmp, residual, p_sig);
	hipLaunchKernelGGL(k_cg_begin, dim3(1), dim3(BLOCK), 0, st, sc, nbs, p_sig, accuracy, useL2Norm);
	MF_LAUNCH_CHECK();
	PcgPlan p;
	MF_TRY(pcg_setup(d, flags, rhs, search, tmp, A0, Ai, Aj, Ak, Aprecond, pc, free_pack, ws, st, &p));

	// ---- iterate, conjugategrad.cpp:238-299; the host only polls `done`, one batch behind the batch it has just queued
	// (every kernel of an iteration returns at once when `done` is already set, so running ahead costs a few empty
	// launches after convergence and keeps the GPU from idling between iterations) ----
	CgScalars h;
	memset(&h, 0, sizeof h);
	h.resNorm = 1e20f;
	// one event pair per device (an event belongs to the device that was current when it was created)
	static thread_local hipEvent_t ev_dev[MAX_DEVICES][2] = {};
	int slot_;
	MF_TRY(device_slot(&slot_));
	hipEvent_t* ev = ev_dev[slot_];
	if (!ev[0]) {
		MF_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
		MF_HIP(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
	}
	CgScalars* hslot = (CgScalars*)ws->host;   // two pinned slots
	// (an external preconditioner -- a multigrid V-cycle -- costs far more than a round trip and its kernels do not read `done`: the
	// host then reads the scalars of every iteration before it queues the next)
	const int batch = ((pc == MF_PC_MICP && mic_mode() == 0) || ext) ? 1 : 4;
	const int be_nb = ((sy + 7) / 8) * ((sz + 7) / 8);      // the sweep's partials (one per bundle) come first, the nbs of the residual update behind them
	int issued = 0, slot = 0, pending = -1;
	while (issued < maxIter) {
		const int todo = (maxIter - issued < batch) ? (maxIter - issued) : batch;
		for (int it = 0; it < todo; it++) {
			int nba = 0, nsig = 0;
			bool beta_done = false;
			MF_TRY(launch_apply_matrix<true>(d, flags, tmp, search, A0, Ai, Aj, Ak, p_dot, sc, st, p.am, &nba));
			hipLaunchKernelGGL(k_cg_alpha, dim3(1), dim3(BLOCK), 0, st, sc, nba, p_dot);
			if (pc == MF_PC_MICP) {
				// (with the skip map but without be_map, the shares it writes behind the sweep's partials are not summed: the sweep has them)
				auto axpy = p.am.skip.on() ? k_cg_axpy_r<false, true> : k_cg_axpy_r<false, false>;
				hipLaunchKernelGGL(axpy, dim3(nbs), dim3(BLOCK), 0, st, n, sc, residual, tmp, p_mm, p_res, p.am.skip, sx, sy, p_sig + be_nb, p.am.nt);
				MicSweep fwd = p.sweep;
				MF_TRY(mic_sweep(1, d, flags, tmp, residual, Aprecond, Ai, Aj, Ak, sc, st, &fwd));
				// sigma_new = dot(tmp, residual) comes out of the backward sweep's write-back (one partial per row bundle); the shares of
				// the bundles the sweeps leave out: from the residual update above, behind the sweep's partials
				// ... and the beta step is the tail of the sweep's last workgroup (one launch less per iteration)
				MicSweep bwd = p.sweep;
				bwd.dotpart = p_sig;
				bwd.empty_ext = p.be_map != nullptr;
				bwd.tail = BetaTail{sc, nbs, p_mm, p_res, p.be_map ? nbs : 0};
				MF_TRY(mic_sweep(2, d, flags, tmp, residual, Aprecond, Ai, Aj, Ak, sc, st, &bwd));
				nsig = bwd.ndot;
				beta_done = bwd.tail_done;
				if (p.be_map) {
					if (nsig != be_nb) return fail("mf_cg_solve: the backward sweep wrote %d dot partials, %d expected", nsig, be_nb);
					nsig += nbs;
				}
			} else if (ext) {
				hipLaunchKernelGGL((k_cg_axpy_r<false>), dim3(nbs), dim3(BLOCK), 0, st, n, sc, residual, tmp, p_mm, p_res);
				MF_TRY(ext->apply(ext->ctx, tmp, residual, st));
			} else {
				hipLaunchKernelGGL((k_cg_axpy_r<true>), dim3(nbs), dim3(BLOCK), 0, st, n, sc, residual, tmp, p_mm, p_res);
			}
			if (nsig == 0) {
				hipLaunchKernelGGL(k_cg_dot, dim3(nbs), dim3(BLOCK), 0, st, n, sc, tmp, residual, p_sig);
				nsig = nbs;
			}
			if (!beta_done) hipLaunchKernelGGL(k_cg_beta, dim3(1), dim3(BLOCK), 0, st, sc, nbs, p_mm, p_res, nsig, p_sig);
			auto update = p.am.skip.on() ? k_cg_update_search_x<true> : k_cg_update_search_x<false>;
			hipLaunchKernelGGL(update, dim3(nbs), dim3(BLOCK), 0, st, n, sc, dst, search, tmp, p.am.skip, sx, sy, p.am.nt);
		}
		MF_LAUNCH_CHECK();
		issued += todo;
		MF_HIP(hipMemcpyAsync(&hslot[slot], sc, sizeof(CgScalars), hipMemcpyDeviceToHost, st));
		MF_HIP(hipEventRecord(ev[slot], st));
		if (ext) pending = slot;
		if (pending >= 0) {
			MF_HIP(hipEventSynchronize(ev[pending]));
			memcpy(&h, &hslot[pending], sizeof h);
			if (h.done || h.diverged) break;
		}
		pending = slot;
		slot ^= 1;
	}
	// the final state, after everything that was queued
	MF_HIP(hipMemcpyAsync(&hslot[0], sc, sizeof(CgScalars), hipMemcpyDeviceToHost, st));
	MF_HIP(hipStreamSynchronize(st));
	memcpy(&h, &hslot[0], sizeof h);
	out_host[0] = (float)h.iterations;
	out_host[1] = h.resNorm;
	out_host[2] = h.sigma;
	if (pc == MF_PC_MICP) MF_TRY(mic_flow_error(st));
	if (h.diverged) return fail("GridCg::iterate: The CG solver diverged, residual norm > 1e30, stopping.");
	return 0;
}

namespace mf {
int cg_solve_external(const Dim& d, const int32_t* flags, float* dst, const float* rhs, float* residual, float* search, float* tmp,
                      const float* A0, const float* Ai, const float* Aj, const float* Ak, const PcExternal* ext, float accuracy, int maxIter,
                      int useL2Norm, float* out_host, void* stream) {
	if (!(al16(dst) && al16(rhs) && al16(residual) && al16(search) && al16(tmp))) return fail("cg_solve_external: work grids must be 16-byte aligned");
	if (maxIter <= 0) return cg_no_iterations(out_host);
	return cg_solve_core(d, flags, dst, rhs, residual, search, tmp, A0, Ai, Aj, Ak, nullptr, MF_PC_MGP, accuracy, maxIter, useL2Norm, out_host, stream,
	                     nullptr, ext);
}
}  // namespace mf

extern "C" {

int mf_apply_matrix(int sx, int sy, int sz, const int32_t* flags, float* dst, const float* src, const float* A0,
                    const float* Ai, const float* Aj, const float* Ak, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	bool a0_packed = false;
	const unsigned char* pk = mic_pack_user(flags, A0, Ai, Aj, Ak, &a0_packed);
	return launch_apply_matrix<false>(d, flags, dst, src, A0, Ai, Aj, Ak, nullptr, nullptr, (hipStream_t)stream, AmOpts{pk, a0_packed});
}

static int time_apply_matrix(int sx, int sy, int sz, const int32_t* flags, float* dst, const float* src, const float* A0,
                             const float* Ai, const float* Aj, const float* Ak, int reps, double* avg_us, void* stream, bool packed) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	AmOpts am;
	if (packed) {
		MF_TRY(mic_pack_query(d, flags, A0, Ai, Aj, Ak, &am.pack, &am.a0_packed, st));
		if (!am.pack) return fail("mf_time_apply_matrix_packed: no packed coefficients for these grids (call mf_mic_init on them; the off-diagonals must all be +0 or -1)");
	}
	hipEvent_t e0, e1;
	MF_HIP(hipEventCreate(&e0));
	MF_HIP(hipEventCreate(&e1));
	for (int i = 0; i < 3; i++) MF_TRY(launch_apply_matrix<false>(d, flags, dst, src, A0, Ai, Aj, Ak, nullptr, nullptr, st, am));
	MF_HIP(hipEventRecord(e0, st));
	for (int i = 0; i < reps; i++) MF_TRY(launch_apply_matrix<false>(d, flags, dst, src, A0, Ai, Aj, Ak, nullptr, nullptr, st, am));
	MF_HIP(hipEventRecord(e1, st));
	MF_HIP(hipEventSynchronize(e1));
	float ms = 0.f;
	MF_HIP(hipEventElapsedTime(&ms, e0, e1));
	*avg_us = (double)ms * 1000.0 / (reps > 0 ? reps : 1);
	(void)hipEventDestroy(e0);
	(void)hipEventDestroy(e1);
	return 0;
}
int mf_time_apply_matrix(int sx, int sy, int sz, const int32_t* flags, float* dst, const float* src, const float* A0,
                         const float* Ai, const float* Aj, const float* Ak, int reps, double* avg_us, void* stream) {
	return time_apply_matrix(sx, sy, sz, flags, dst, src, A0, Ai, Aj, Ak, reps, avg_us, stream, false);
}
int mf_time_apply_matrix_packed(int sx, int sy, int sz, const int32_t* flags, float* dst, const float* src, const float* A0,
                                const float* Ai, const float* Aj, const float* Ak, int reps, double* avg_us, void* stream) {
	return time_apply_matrix(sx, sy, sz, flags, dst, src, A0, Ai, Aj, Ak, reps, avg_us, stream, true);
}

int mf_make_laplace_matrix(int sx, int sy, int sz, const int32_t* flags, float* A0, float* Ai, float* Aj, float* Ak,
                           const float* fractions, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_make_laplace, dim3((unsigned)((d.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, A0, Ai, Aj, Ak, fractions);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_make_rhs(int sx, int sy, int sz, const int32_t* flags, float* rhs, const float* vel, const float* perCellCorr,
                const float* fractions, const float* obvel, const float* phi, const float* curv, float surfTens,
                float gfClamp, int32_t* cnt_host, double* sum_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	hipStream_t st = (hipStream_t)stream;
	const int nb = blocks_for(d.n, BLOCK, 2048);
	hipLaunchKernelGGL(k_make_rhs, dim3(nb), dim3(BLOCK), 0, st, d, flags, rhs, vel, perCellCorr, fractions, obvel, phi, curv, surfTens, gfClamp, ws->partials);
	hipLaunchKernelGGL(k_sum2_finish, dim3(1), dim3(BLOCK), 0, st, nb, ws->partials, ws->partials + MAX_BLOCKS, (double*)ws->scalars);
	MF_LAUNCH_CHECK();
	if (cnt_host || sum_host) {
		MF_HIP(hipMemcpyAsync(ws->host, ws->scalars, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
		MF_HIP(hipStreamSynchronize(st));
		const double* h = (const double*)ws->host;
		if (sum_host) *sum_host = h[0];
		if (cnt_host) *cnt_host = (int32_t)h[1];
	}
	return 0;
}

int mf_apply_ghost_fluid_diagonal(int sx, int sy, int sz, float* A0, const int32_t* flags, const float* phi, float gfClamp, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_ghost_fluid_diag, dim3((unsigned)((d.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, d, A0, flags, phi, gfClamp);
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_correct_velocity(int sx, int sy, int sz, const int32_t* flags, float* vel, const float* pressure, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_correct_velocity, dim3((unsigned)((d.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, d, flags, vel, pressure);
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_correct_velocity_ghost_fluid(int sx, int sy, int sz, float* vel, const int32_t* flags, const float* pressure,
                                    const float* phi, float gfClamp, const float* curv, float surfTens, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_correct_velocity_gf, dim3((unsigned)((d.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, d, vel, flags, pressure, phi, gfClamp, curv, surfTens);
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_replace_clamped_ghost_fluid_vels(int sx, int sy, int sz, float* vel, const int32_t* flags, const float* pressure,
                                        const float* phi, float gfClamp, void* stream) {
	(void)pressure;
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipLaunchKernelGGL(k_replace_clamped_gf, dim3((unsigned)((d.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, d, vel, flags, phi, gfClamp);
	MF_LAUNCH_CHECK();
	return 0;
}
int mf_fix_pressure(int sx, int sy, int sz, int64_t fixPidx, float value, float* rhs, float* A0, float* Ai, float* Aj, float* Ak, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	if (fixPidx - d.Y < 0 || fixPidx + d.Y >= d.n || fixPidx - d.Z < 0 || fixPidx + d.Z >= d.n) return fail("fixPressure: cell %lld on the domain border", (long long)fixPidx);
	hipLaunchKernelGGL(k_fix_pressure, dim3(1), dim3(1), 0, (hipStream_t)stream, d, fixPidx, value, rhs, A0, Ai, Aj, Ak);
	MF_LAUNCH_CHECK();
	return 0;
}

// ---- fused pieces of the z-slab PCG (mantaflow_amd/slab.py): scalars live in a CgScalars-layout device block ----
int mf_apply_matrix_dot_dev(int sx, int sy, int sz, const int32_t* flags, float* dst, const float* src, const float* A0,
                            const float* Ai, const float* Aj, const float* Ak, int k0, int k1, const void* scalars, double* dot_dev,
                            void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	if (k0 < 0 || k1 > sz || k0 > k1) return fail("mf_apply_matrix_dot_dev: invalid plane range");
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const CgScalars* sc = (const CgScalars*)scalars;
	int nb = 0;
	bool ranged = false;
	AmOpts am;
	am.pack = mic_pack_user(flags, A0, Ai, Aj, Ak, &am.a0_packed);
	am.dk0 = k0;
	am.dk1 = k1;
	MF_TRY(launch_apply_matrix<true>(d, flags, dst, src, A0, Ai, Aj, Ak, ws->partials, sc, st, am, &nb, &ranged));
	if (!ranged) {
		// the fallback kernels sum over the whole grid: redo the dot over the requested planes
		const int64_t XY = (int64_t)sx * sy, n = (int64_t)(k1 - k0) * XY;
		nb = blocks_for(n >> 2, BLOCK, 2048);
		hipLaunchKernelGGL(k_cg_dot, dim3(nb), dim3(BLOCK), 0, st, n, sc, dst + k0 * XY, src + k0 * XY, ws->partials);
	}
	return launch_sum_finish(nb, ws->partials, dot_dev, st);
}
int mf_cg_slab_axpy2(int64_t n, const void* scalars, float* x, const float* search, float* residual, const float* tmp,
                     double* maxabs_dev, void* stream) {
	if (n <= 0) return 0;
	hipStream_t st = (hipStream_t)stream;
	if (!(al16(x) && al16(search) && al16(residual) && al16(tmp))) {
		// views that do not start on a 16-byte boundary (odd plane sizes): the unfused sequence
		const float* alpha_dev = &((const CgScalars*)scalars)->alpha;
		MF_TRY(mf_grid_scaled_add_dev(n, x, search, alpha_dev, 1.f, stream));
		MF_TRY(mf_grid_scaled_add_dev(n, residual, tmp, alpha_dev, -1.f, stream));
		return mf_grid_max_abs_dev_f64(n, residual, maxabs_dev, stream);
	}
	Workspace* ws;
	MF_TRY(get_workspace(&ws));
	const int nb = blocks_for(n >> 2, BLOCK, 2048);
	hipLaunchKernelGGL(k_cg_axpy2, dim3(nb), dim3(BLOCK), 0, st, n, (const CgScalars*)scalars, x, search, residual, (float*)tmp, ws->fpartials, ws->partials + MAX_BLOCKS);
	return launch_maxabs_finish(nb, ws->fpartials, maxabs_dev, nullptr, st);
}

int mf_diffusion_matrix(int sx, int sy, int sz, const int32_t* flags, float* A0, float* Ai, float* Aj, float* Ak, float alpha,
                        void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const int64_t n = (int64_t)sx * sy * sz;
	hipLaunchKernelGGL(k_diffusion_matrix, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, n, flags, A0, Ai, Aj, Ak, alpha);
	MF_LAUNCH_CHECK();
	return 0;
}

int mf_cg_last_shortcut(int32_t* out) {
	out[0] = g_last_shortcut[0];
	out[1] = g_last_shortcut[1];
	out[2] = g_last_shortcut[2];
	return 0;
}
int mf_cg_solve(int sx, int sy, int sz, const int32_t* flags, float* dst, const float* rhs, float* residual, float* search,
                float* tmp, const float* A0, const float* Ai, const float* Aj, const float* Ak, float* Aprecond, int pc,
                float accuracy, int maxIter, int useL2Norm, float* out_host, void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	if (pc != MF_PC_NONE && pc != MF_PC_MICP) return fail("GridCg<APPLYMAT>::setICPreconditioner: Invalid method specified.");
	if (pc == MF_PC_MICP && !d.is3d) pc = MF_PC_NONE;  // conjugategrad.cpp:315-321
	if (!(al16(dst) && al16(rhs) && al16(residual) && al16(search) && al16(tmp))) return fail("mf_cg_solve: work grids must be 16-byte aligned");
	if (maxIter <= 0) return cg_no_iterations(out_host);
	// Row lengths that are not a multiple of 8 (benchmark_dam.py: 3.2 res + 8) would take the sweeps and ApplyMatrix off their
	// 16-byte paths and off the packed coefficient bytes (379 x 356 x 124: 0.83 instead of ~0.5 ms per iteration).  The PCG then
	// runs on its own copy of the system with the rows padded to the next multiple of 8: pad cells are obstacle cells with zero
	// coefficients and zero rhs, so they pass zeros through ApplyMatrix and the sweeps and add zeros to every reduction -- the
	// iterates of the fluid cells are those of the unpadded system.  (A fluid cell in the last column, which MakeLaplaceMatrix
	// never writes, would read the pad cell instead of the next row's first cell, both times a zero coefficient: the same value.)
	// If the padded copy cannot be allocated, the solve runs unpadded on the caller's grids (the path of every sx % 8 == 0 system).
	if (pc == MF_PC_MICP && (sx % 8) != 0 && sx >= 16) {
		const int px = (sx + 7) & ~7;
		const int64_t rows = (int64_t)sy * sz, np_ = (int64_t)px * rows;
		if (np_ < ((int64_t)1 << 31)) {
			const size_t need = 11 * al256(sizeof(float) * (size_t)np_);
			Arena* a;
			int32_t* p_flags;
			float *p_dst, *p_rhs, *p_res, *p_search, *p_tmp, *p_A0, *p_Ai, *p_Aj, *p_Ak, *p_Ap;
			if (arena_reserve(g_pad, need, &a) == 0) {
				Cutter c(a->p, need);
				MF_TRY(c.take((size_t)np_, &p_flags, &p_dst, &p_rhs, &p_res, &p_search, &p_tmp, &p_A0, &p_Ai, &p_Aj, &p_Ak, &p_Ap));
				// doInit overwrites dst, residual and search, but not the non-fluid cells of tmp: the sweeps never write them,
				// ApplyMatrix copies search there, and the dots run over all cells -- the caller's tmp goes in with the system
				// (k_pad_system writes every element of the seven slices it is given)
				for (float* q : {p_dst, p_res, p_search, p_Ap}) MF_HIP(hipMemsetAsync(q, 0, sizeof(float) * np_, st));
				hipLaunchKernelGGL(k_pad_system, dim3(blocks_for(np_, BLOCK, 4096)), dim3(BLOCK), 0, st, sx, px, np_, flags, rhs, tmp, A0, Ai, Aj, Ak,
				                   p_flags, p_rhs, p_tmp, p_A0, p_Ai, p_Aj, p_Ak);
				MF_LAUNCH_CHECK();
				MF_TRY(mf_cg_solve(px, sy, sz, p_flags, p_dst, p_rhs, p_res, p_search, p_tmp, p_A0, p_Ai, p_Aj, p_Ak, p_Ap, pc, accuracy,
				                   maxIter, useL2Norm, out_host, stream));
				hipLaunchKernelGGL(k_unpad, dim3(blocks_for(d.n, BLOCK, 4096)), dim3(BLOCK), 0, st, sx, px, d.n, p_dst, dst);
				MF_LAUNCH_CHECK();
				return 0;
			}
			(void)hipGetLastError();      // the reservation failed (the block is then nullptr / 0): clear its error, solve unpadded
		}
	}
	return cg_solve_core(d, flags, dst, rhs, residual, search, tmp, A0, Ai, Aj, Ak, Aprecond, pc, accuracy, maxIter, useL2Norm, out_host, stream, nullptr);
}

int mf_solve_pressure_fused(int sx, int sy, int sz, const int32_t* flags, const float* vel, float* pressure, float* rhs, float* residual,
                            float* search, float* tmp, float* Aprecond, float accuracy, int maxIter, int useL2Norm, float* out_host,
                            void* stream) {
	MF_TRY(check_dim(sx, sy, sz));
	const Dim d = mkdim(sx, sy, sz);
	hipStream_t st = (hipStream_t)stream;
	if (!d.is3d || (sx % 8) != 0 || mic_mode() != 2) return fail("mf_solve_pressure_fused: needs a 3D grid with sx % 8 == 0 and the \"rows\" sweeps");
	if (!(al16(flags) && al16(vel) && al16(pressure) && al16(rhs) && al16(residual) && al16(search) && al16(tmp) && al16(Aprecond)))
		return fail("mf_solve_pressure_fused: grids must be 16-byte aligned");
	unsigned char* pack;
	int* bempty;
	int nbj;
	MF_TRY(mic_fused_begin(d, st, &pack, &bempty, &nbj));
	const int64_t nthr = (int64_t)(sx >> 2) * sy * sz;
	hipLaunchKernelGGL(k_setup_fused, dim3((unsigned)((nthr + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, d, flags, vel, rhs, pack, bempty, nbj);
	MF_LAUNCH_CHECK();
	MF_TRY(mic_fused_finish(d, flags, Aprecond, st));
	if (maxIter <= 0) return cg_no_iterations(out_host);
	// the sweeps never write a non-fluid cell of tmp: it has to start from zeros (a fresh temp grid in the reference)
	MF_HIP(hipMemsetAsync(tmp, 0, sizeof(float) * d.n, st));
	return cg_solve_core(d, flags, pressure, rhs, residual, search, tmp, nullptr, nullptr, nullptr, nullptr, Aprecond, MF_PC_MICP, accuracy, maxIter,
	                     useL2Norm, out_host, stream, pack);
}


// the stretches of a z-slab PCG iteration between two communication points, queued with one call each (CgScalars layout: sigma,
// alpha, nalpha, beta, resNorm at floats 0, 1, 2, 3, 4); x += alpha * search rides on the search update as in mf_cg_solve
int mf_cg_slab_after_dp(const double* gathered, int world, void* scalars, const int32_t* state_dev, int64_t own_off, int64_t n_own,
                        float* residual, float* tmp, double* maxabs_dev, int sx, int sy, int sz,
                        const int32_t* flags, const float* Aprecond, const float* Ai, const float* Aj, const float* Ak, double* dot_dev,
                        void* stream) {
	hipStream_t st = (hipStream_t)stream;
	CgScalars* sc = (CgScalars*)scalars;
	float* r = residual + own_off;
	float* t = tmp + own_off;
	const bool one_launch = n_own > 0 && state_dev && al16(r) && al16(t);
	if (!one_launch) hipLaunchKernelGGL(k_slab_alpha_x, dim3(1), dim3(1), 0, st, gathered, world, sc, state_dev);
	if (n_own > 0) {
		if (one_launch) {
			Workspace* ws;
			MF_TRY(get_workspace(&ws));
			const int nb = blocks_for(n_own >> 2, BLOCK, 2048);
			// the alpha step rides in the residual update (every block forms it from the gathered rows)
			hipLaunchKernelGGL(k_slab_axpy_r, dim3(nb), dim3(BLOCK), 0, st, n_own, gathered, world, sc, state_dev, r, t, ws->fpartials, n_own > PCG_NT_CELLS ? 1 : 0);
			MF_LAUNCH_CHECK();
			// max |r| of these partials and dot(tmp, r): folded by the last workgroup of the backward sweep (no one-block launches)
			MF_TRY(check_dim(sx, sy, sz));
			const Dim d = mkdim(sx, sy, sz);
			if (!d.is3d) return fail("mICP only supports 3D grids so far");
			return mic_apply_dot_fold(d, flags, tmp, residual, Aprecond, Ai, Aj, Ak, dot_dev, nb, ws->fpartials, maxabs_dev, sc, st);
		} else {
			// views that do not start on a 16-byte boundary (odd plane sizes), or no stop state: the unfused sequence (a no-op once stopped)
			Workspace* ws;
			MF_TRY(get_workspace(&ws));
			const int nb = blocks_for(n_own, BLOCK, 2048);
			hipLaunchKernelGGL(k_slab_axpy_r_scalar, dim3(nb), dim3(BLOCK), 0, st, n_own, sc, r, t, ws->fpartials);
			MF_TRY(launch_maxabs_finish(nb, ws->fpartials, maxabs_dev, nullptr, st));
		}
	}
	return mf_mic_apply_dot_dev(sx, sy, sz, flags, tmp, residual, Aprecond, Ai, Aj, Ak, dot_dev, stream);
}
int mf_cg_slab_after_zr(const double* gathered, int world, void* scalars, float accuracy, int iter, int32_t* state_dev, int64_t own_off,
                        int64_t n_own, float* x, float* search, const float* tmp, void* stream) {
	hipStream_t st = (hipStream_t)stream;
	CgScalars* sc = (CgScalars*)scalars;
	float* xs = x + own_off;
	float* s = search + own_off;
	const float* t = tmp + own_off;
	if (n_own > 0 && state_dev && al16(xs) && al16(s) && al16(t)) {
		// the beta step and the stopping test ride in the search update
		hipLaunchKernelGGL(k_slab_update_search_x, dim3(blocks_for(n_own >> 2, BLOCK, 2048)), dim3(BLOCK), 0, st, n_own, gathered, world, sc,
		                   accuracy, iter, state_dev, xs, s, t, n_own > PCG_NT_CELLS ? 1 : 0);
		MF_LAUNCH_CHECK();
		return 0;
	}
	hipLaunchKernelGGL(k_slab_beta_x, dim3(1), dim3(1), 0, st, gathered, world, sc, accuracy, iter, state_dev);
	if (n_own <= 0) return 0;
	hipLaunchKernelGGL(k_cg_update_search_x_scalar, dim3(blocks_for(n_own, BLOCK, 2048)), dim3(BLOCK), 0, st, n_own, sc, xs, s, t);
	MF_LAUNCH_CHECK();
	return 0;
}

}  // extern "C"
