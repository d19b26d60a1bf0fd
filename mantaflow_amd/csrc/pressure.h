// pressure.h -- what pressure.hip (PCG loop) and mic.hip (MIC(0) preconditioner sweeps) share.
#pragma once
#include "common.h"

// device-resident PCG scalars (GridCg members, conjugategrad.h:95-112): written by one-block kernels, read by every
// kernel of an iteration; `done` makes the kernels of iterations queued after convergence return at once
struct CgScalars {
	float sigma, alpha, nalpha, beta, resNorm, dp, sigmaNew, accuracy;
	int iterations, done, diverged, useL2;
	int xpending;     // this iteration's dst += alpha * search is still to be done (by k_cg_update_search_x)
	float sigmaPrev;  // z-slab solver: sigma as the alpha step saw it (the beta step's divisor while block 0 of the same kernel writes sigma)
};

// residual norm (max-norm from the min / max lo, hi, or the sum of squares ss), convergence test, beta from dd = dot(tmp, residual),
// divergence flag (the host finishes the iteration's search update, then reports).  conjugategrad.cpp:268-295; one thread
__device__ __forceinline__ void cg_beta_step(CgScalars* sc, bool l2, float lo, float hi, double ss, double dd) {
	float resNorm;
	if (l2) resNorm = (float)ss;
	else resNorm = mf::maxabs(lo, hi);
	sc->resNorm = resNorm;
	if (resNorm < sc->accuracy) {
		sc->sigma = resNorm;
		sc->done = 1;
	} else {
		const float sigmaNew = (float)dd;
		sc->beta = sigmaNew / sc->sigma;
		sc->sigmaNew = sigmaNew;
		sc->sigma = sigmaNew;
		if (!((double)resNorm < 1e35)) sc->diverged = 1;
	}
}

// ---- the packed coefficient byte of a cell (k_mic_pack, k_setup_fused; only offered when every off-diagonal is exactly +0 or -1):
// fluid flag, "Ai / Aj / Ak is -1" bits, and in bits 4-7 the diagonal A0 where it is a small integer.  A zero byte is a non-fluid cell
// without couplings (k_pack_xrange).  Decoders of one byte, and of a 32-bit word of four cells (x, y, z, w = bytes 0..3).
constexpr unsigned PK_FLUID = 1u, PK_AI = 2u, PK_AJ = 4u, PK_AK = 8u, PK_A0_MAX = 15u;
constexpr int PK_A0_SHIFT = 4;
constexpr unsigned PK_WORD = 0x01010101u;      // times a bit: that bit of all four bytes of a word
__host__ __device__ __forceinline__ unsigned pk_make(bool fluid, bool ai, bool aj, bool ak, unsigned a0) {
	return (fluid ? PK_FLUID : 0u) | (ai ? PK_AI : 0u) | (aj ? PK_AJ : 0u) | (ak ? PK_AK : 0u) | (a0 << PK_A0_SHIFT);
}
__device__ __forceinline__ bool pk_fluid(unsigned b) { return (b & PK_FLUID) != 0; }
template <unsigned BIT>
__device__ __forceinline__ float pk_coef(unsigned b) { return (b & BIT) ? -1.f : 0.f; }
__device__ __forceinline__ float pk_a0(unsigned b) { return (float)((b >> PK_A0_SHIFT) & PK_A0_MAX); }
__device__ __forceinline__ int4 unpack_flags(unsigned w) {
	return make_int4((w & PK_FLUID) ? MF_FLUID : 0, (w & (PK_FLUID << 8)) ? MF_FLUID : 0, (w & (PK_FLUID << 16)) ? MF_FLUID : 0,
	                 (w & (PK_FLUID << 24)) ? MF_FLUID : 0);
}
template <unsigned BIT>
__device__ __forceinline__ float4 unpack_coef(unsigned w) {
	return make_float4(pk_coef<BIT>(w), pk_coef<(BIT << 8)>(w), pk_coef<(BIT << 16)>(w), pk_coef<(BIT << 24)>(w));
}
__device__ __forceinline__ float4 unpack_a0(unsigned w) { return make_float4(pk_a0(w), pk_a0(w >> 8), pk_a0(w >> 16), pk_a0(w >> 24)); }

// ---- liquid scenes: what the kernels of a PCG iteration leave out.  Most 8 x 8 bundles of rows hold no fluid cell, and the packed
// system has an x-range outside of which every byte is zero; where rhs and the work grids are +0 there (k_cg_outside_zero counts the
// exceptions into outside_bad[0], once per solve) every vector stays +0 there and nothing needs to be read or written.  By value.
struct SkipMap {
	const int* bempty = nullptr;       // 1 per empty bundle (mic_empty_map), nbj bundles per row of bundles; nullptr: no map, skip nothing
	int nbj = 0;
	const int* outside_bad = nullptr;  // device verdict on the premise: skip only while outside_bad[0] == 0
	const int* xr = nullptr;           // {first, one past the last} cell of the packed system's x-range (k_pack_xrange); nullptr: whole rows
	// the x-range as skipped by: rounded outwards to chunks of 8 cells (what the trimmed MIC sweeps leave out)
	struct XRange {
		int lo, hi;
		__host__ __device__ bool outside(int x) const { return x < lo || x >= hi; }
	};
	__host__ __device__ static XRange rounded(int lo, int hi) { return XRange{lo & ~7, (hi + 7) & ~7}; }
	__host__ __device__ bool on() const { return bempty != nullptr; }
	// the members below: device side, of a map that is on()
	__device__ bool active() const { return outside_bad[0] == 0; }
	__device__ XRange range(int sx) const { return xr ? rounded(xr[0], xr[1]) : XRange{0, sx}; }
	__device__ bool empty_bundle(int j, int k) const { return bempty[(k >> 3) * nbj + (j >> 3)] != 0; }
};
// row (j, k) and first cell x of quad q of a grid with sx % 4 == 0 (a quad lies in one row)
__device__ __forceinline__ void quad_cell(int64_t q, int sx, int sy, int& j, int& k, int& x) {
	const int64_t row = (4 * q) / sx;
	j = (int)(row % sy);
	k = (int)(row / sy);
	x = (int)(4 * q - row * sx);
}

// ---- four cells at a time: the arithmetic of the PCG's vector kernels, component by component in x, y, z, w order
__device__ __forceinline__ float4 axpy4(float4 a, float f, float4 b) {      // a + f * b, two roundings each
	a.x = a.x + f * b.x; a.y = a.y + f * b.y; a.z = a.z + f * b.z; a.w = a.w + f * b.w;
	return a;
}
// (accumulators go in and come out by value: by reference the kernels compile to other code)
__device__ __forceinline__ float min4(float lo, float4 r) { return fminf(fminf(lo, r.x), fminf(r.y, fminf(r.z, r.w))); }
__device__ __forceinline__ float max4(float hi, float4 r) { return fmaxf(fmaxf(hi, r.x), fmaxf(r.y, fmaxf(r.z, r.w))); }
__device__ __forceinline__ double sumsq4(double ss, float4 r) {
	ss += (double)r.x * (double)r.x;
	ss += (double)r.y * (double)r.y;
	ss += (double)r.z * (double)r.z;
	ss += (double)r.w * (double)r.w;
	return ss;
}
// GridDotProduct (conjugategrad.cpp:175-178): fp32 products, accumulated in fp64
__device__ __forceinline__ double dot4(double acc, float4 a, float4 b) {
	const float p0 = a.x * b.x, p1 = a.y * b.y, p2 = a.z * b.z, p3 = a.w * b.w;
	acc += (double)p0;
	acc += (double)p1;
	acc += (double)p2;
	acc += (double)p3;
	return acc;
}
__device__ __forceinline__ float4 ld4(const float* p, bool nt) { return nt ? mf::ld_nt4(p) : *(const float4*)p; }
__device__ __forceinline__ void st4(float* p, float4 v, bool nt) {
	if (nt) mf::st_nt4(p, v);
	else *(float4*)p = v;
}

// the beta step of the PCG (k_cg_beta: residual norm, convergence test, beta; conjugategrad.cpp:268-295) as the tail of the backward MIC
// sweep's last workgroup: the partials of the residual update (an earlier kernel) and the nsig dot partials (this launch's, plus what
// the caller appended behind them)
struct BetaTail {
	CgScalars* sc;            // nullptr: no tail
	int nbr;                  // blocks of the residual update
	const float* fpart;       // their min / max pairs
	const double* dpart_res;  // their sums of squares (L2 norm)
	int nsig;                 // dot partials to fold
	// sc == nullptr and sum_out set: the z-slab solver's variant -- no beta step here (the scalars of all ranks are gathered first), the
	// last workgroup only folds: *sum_out = sum of the nsig dot partials (launch_sum_finish's order) and, with nbr > 0, *maxabs_out =
	// max |fpart| unless live->done (launch_maxabs_finish)
	double* sum_out;
	double* maxabs_out;
	const CgScalars* live;
};
// options of one MIC sweep (mic_sweep), filled by the caller; the outputs are written by the call
struct MicSweep {
	// backward sweep in "rows" mode: GridDotProduct(dst, var1) fused into the write-back, one partial per bundle into dotpart (summed
	// in index order by the caller)
	double* dotpart = nullptr;
	// the caller sums the dot shares of the bundles the sweep leaves out itself (mic_empty_map tells which), their entries come out 0
	bool empty_ext = false;
	// the beta step (or the z-slab solver's fold) as the tail of the sweep's last workgroup, where the sweep can take it
	BetaTail tail = BetaTail{nullptr, 0, nullptr, nullptr, 0};
	// the sweeps of the registered system (on its packed bytes) cover the cells [trim_xoff, trim_xoff + 8 trim_chunks) of every row
	// only (0 chunks: whole rows).  The caller guarantees that every cell outside has a zero packed byte (non-fluid, no couplings) and
	// the value +0 in the swept grid, and accounts for nothing of them in the fused dot (their products are +0).
	int trim_xoff = 0, trim_chunks = 0;
	int ndot = 0;             // out: partials written to dotpart (0: the active mode cannot fuse the dot -- the caller runs its own)
	bool tail_done = false;   // out: the tail was folded into the sweep
};
// a preconditioner that lives outside pressure.hip / mic.hip (multigrid.hip: PC_MGP).  init: once in doInit, before the first
// apply (InitPrecondition...); apply: dst = M^-1 src on whole grids
struct PcExternal {
	int (*init)(void* ctx, const float* A0, const float* Ai, const float* Aj, const float* Ak, float accuracy, hipStream_t st);
	int (*apply)(void* ctx, float* dst, const float* src, hipStream_t st);
	void* ctx;
};
namespace mf {
// mf_cg_solve's doInit + iterate loop (cg_solve_core: the same ApplyMatrix, fp64 dots and fused updates) around an external preconditioner
int cg_solve_external(const Dim& d, const int32_t* flags, float* dst, const float* rhs, float* residual, float* search, float* tmp,
                      const float* A0, const float* Ai, const float* Aj, const float* Ak, const PcExternal* ext, float accuracy, int maxIter,
                      int useL2Norm, float* out_host, void* stream);
// mode 0: InitPreconditionModifiedIncompCholesky2 (dst := Aprecond, var1 := A0); 1 / 2: forward / backward substitution
// of ApplyPreconditionModifiedIncompCholesky2.  sc (nullable): skip when sc->done.  opt (nullable): see MicSweep
int mic_sweep(int mode, const Dim& d, const int32_t* flags, float* dst, const float* var1, const float* Ap, const float* Ai,
              const float* Aj, const float* Ak, const CgScalars* sc, hipStream_t st, MicSweep* opt = nullptr);
// forward + backward substitution with dot(dst, var1) -> *dot_dev and (nbr > 0) the max |.| of the nbr min / max pairs in fpart ->
// *maxabs_dev (skipped once live->done): folded by the backward sweep's last workgroup where the active mode allows, by one-block
// kernels behind it otherwise
int mic_apply_dot_fold(const Dim& d, const int32_t* flags, float* dst, const float* var1, const float* Ap, const float* Ai,
                       const float* Aj, const float* Ak, double* dot_dev, int nbr, const float* fpart, double* maxabs_dev,
                       const CgScalars* live, hipStream_t st);
// the empty-bundle map of the system registered for (flags, Ap, Aj, Ak) in "rows" mode, if that system has empty bundles (one small
// read-back per system); *bempty = nullptr otherwise.  *several: the sweeps draw several bundles per workgroup -- then the shares of the
// empty bundles in the fused dot are worth summing elsewhere (MicSweep::empty_ext); otherwise the map is only what the vector kernels of
// the PCG skip by
int mic_empty_map(const Dim& d, const int32_t* flags, const float* Ap, const float* Aj, const float* Ak, const int** bempty, int* nbj, bool* several,
                  hipStream_t st);
// packed {fluid, Ai, Aj, Ak} bytes built by the last mf_mic_init for exactly these grids (nullptr when unavailable / not exact);
// synchronises the stream once.  *a0_packed: bits 4-7 of every byte hold the (small integer) diagonal A0 of these grids as well
int mic_pack_query(const Dim& d, const int32_t* flags, const float* A0, const float* Ai, const float* Aj, const float* Ak,
                   const unsigned char** pack, bool* a0_packed, hipStream_t st);
// packed bytes built by mf_pack_matrix for exactly these grids, or nullptr (no synchronisation); *a0_packed: they carry this A0
const unsigned char* mic_pack_user(const int32_t* flags, const float* A0, const float* Ai, const float* Aj, const float* Ak, bool* a0_packed);
int mic_mode();          // the requested sweep mode (mf_set_mic_mode): 0 levels, 2 rows
// matrix-free set-up of mf_solve_pressure_fused: buffers of the system handle (empty-bundle map preset to 1 = empty), then the MIC
// factor from the packed bytes and the registration of (flags, Aprecond) as a system without coefficient arrays
int mic_fused_begin(const Dim& d, hipStream_t st, unsigned char** pack, int** bempty, int* nbj);
int mic_fused_finish(const Dim& d, const int32_t* flags, float* Aprecond, hipStream_t st);
int mic_flow_error(hipStream_t st);    // reads (and clears) the deadlock-guard flag of the single-launch sweeps after the work queued on st; synchronises st
}  // namespace mf
