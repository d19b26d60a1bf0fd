// reduce.h -- the two-stage device reduction behind every scalar the library hands to the host: a grid-stride kernel writes one partial
// per block, one block folds the partials, an epilogue stores the result.  The order is fixed, so a result is the same bits run to run
// (tests/reduce_model.py restates it):
//   thread g of the grid takes items g, g + T, g + 2T, ... (T the threads of the grid) -> 6 shuffle-down steps per wave -> the 4 wave
//   results in order -> thread q of the finisher takes partials q, q + 256, ... -> the same block fold.
// The accumulator is always the left operand: fminf / fmaxf of +0 and -0 and of a NaN depend on it.
#pragma once
#include "common.h"
#include <limits>

namespace mf {

// ---- fold policies: T the folded value, identity(), fold(a, b) for a = a (+) b, down() the wave shuffle ----------------------------
template <class S>
struct Sum {      // fp64 sums; int64 sums of int32 terms are exact, whatever the order
	typedef S T;
	static __device__ __forceinline__ T identity() { return S(0); }
	static __device__ __forceinline__ void fold(T& a, T b) { a += b; }
	static __device__ __forceinline__ T down(T v, int o) { return __shfl_down(v, o, 64); }
};
typedef Sum<double> SumF64;
typedef Sum<long long> SumI64;

__device__ __forceinline__ float min_of(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float max_of(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ int min_of(int a, int b) { return min(a, b); }
__device__ __forceinline__ int max_of(int a, int b) { return max(a, b); }

template <class S>
struct Pair {
	S lo, hi;
};
template <class S>
struct MinMax {   // a minimum and a maximum side by side: a partial is the pair {lo, hi}
	typedef Pair<S> T;
	static __device__ __forceinline__ T identity() { return {std::numeric_limits<S>::max(), std::numeric_limits<S>::lowest()}; }
	static __device__ __forceinline__ void fold(T& a, T b) {
		a.lo = min_of(a.lo, b.lo);
		a.hi = max_of(a.hi, b.hi);
	}
	static __device__ __forceinline__ void fold(T& a, S v) { fold(a, T{v, v}); }
	static __device__ __forceinline__ T down(T v, int o) { return {__shfl_down(v.lo, o, 64), __shfl_down(v.hi, o, 64)}; }
};
typedef MinMax<float> MinMaxF32;
typedef MinMax<int32_t> MinMaxI32;

struct MaxF64 {   // of magnitudes: an empty or all-NaN range gives 0
	typedef double T;
	static __device__ __forceinline__ T identity() { return 0.; }
	static __device__ __forceinline__ void fold(T& a, T b) { a = fmax(a, b); }
	static __device__ __forceinline__ T down(T v, int o) { return __shfl_down(v, o, 64); }
};

// ---- block-wide fold for blockDim.x == BLOCK (4 waves); result valid in thread 0.  The leading barrier makes calls in a row safe: the
// shared array of one instance is reused by the next call ----
template <class F>
__device__ __forceinline__ typename F::T block_fold(typename F::T v) {
	__shared__ typename F::T sh[BLOCK / 64];
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) F::fold(v, F::down(v, o));
	const int w = threadIdx.x >> 6;
	__syncthreads();
	if ((threadIdx.x & 63) == 0) sh[w] = v;
	__syncthreads();
	if (threadIdx.x == 0) {
		v = sh[0];
		for (int i = 1; i < (int)(blockDim.x >> 6); i++) F::fold(v, sh[i]);
	}
	return v;
}
__device__ __forceinline__ double block_sum(double v) { return block_fold<SumF64>(v); }
__device__ __forceinline__ void block_minmax(float& lo, float& hi) {
	const Pair<float> r = block_fold<MinMaxF32>({lo, hi});
	lo = r.lo;
	hi = r.hi;
}

// per-thread strided fold over per-block partials with 8 loads in flight (a plain loop serialises one memory round trip per element);
// fixed order -> deterministic
template <class F>
__device__ __forceinline__ typename F::T strided_fold(const typename F::T* __restrict__ p, int nb) {
	typename F::T acc = F::identity();
	int i = threadIdx.x;
	const int S = blockDim.x;
	for (; i + 7 * S < nb; i += 8 * S) {
		typename F::T v[8];
#pragma unroll
		for (int q = 0; q < 8; q++) v[q] = p[i + q * S];
#pragma unroll
		for (int q = 0; q < 8; q++) F::fold(acc, v[q]);
	}
	for (; i < nb; i += S) F::fold(acc, p[i]);
	return acc;
}
__device__ __forceinline__ double strided_sum(const double* __restrict__ p, int nb) { return strided_fold<SumF64>(p, nb); }

// ---- stage 1: K values folded together over n items.  term(idx, acc) folds item idx into acc[0 .. K); gridDim.y selects a component
// (the term reads blockIdx.y).  partials[(blockIdx.y * K + q) * gridDim.x + block] ----
template <class F, int K, class Term>
static __global__ void __launch_bounds__(BLOCK) k_reduce_partials(int64_t n, Term term, typename F::T* __restrict__ partials) {
	typename F::T acc[K];
#pragma unroll
	for (int q = 0; q < K; q++) acc[q] = F::identity();
	for (int64_t idx = blockIdx.x * (int64_t)BLOCK + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * BLOCK) term(idx, acc);
#pragma unroll
	for (int q = 0; q < K; q++) {
		const typename F::T r = block_fold<F>(acc[q]);
		if (threadIdx.x == 0) partials[(blockIdx.y * K + q) * (int64_t)gridDim.x + blockIdx.x] = r;
	}
}
// ---- stage 2: one block per component folds the nb partials of each of its K values; epi(acc) runs in thread 0 (it reads blockIdx.x
// for the component) ----
template <class F, int K, class Epi>
static __global__ void __launch_bounds__(BLOCK) k_reduce_finish(int nb, const typename F::T* __restrict__ partials, Epi epi) {
	typename F::T acc[K];
#pragma unroll
	for (int q = 0; q < K; q++) acc[q] = block_fold<F>(strided_fold<F>(partials + (blockIdx.x * K + q) * (int64_t)nb, nb));
	if (threadIdx.x == 0) epi(acc);
}

// ---- epilogues ----
template <class T, int K = 1>
struct Store {       // as is: out[component * K + q]
	T* out;
	__device__ __forceinline__ void operator()(const T (&acc)[K]) const {
		for (int q = 0; q < K; q++) out[blockIdx.x * K + q] = acc[q];
	}
};
// max |.| of the min / max pair as O; nothing when stopped (nullable; the z-slab solver's iterations queued past the stop) points to a
// non-zero word: *out keeps the value of the stopping iteration
template <class O>
struct StoreMaxAbs {
	O* out;
	const int* stopped;
	__device__ __forceinline__ void operator()(const Pair<float> (&acc)[1]) const {
		if (!(stopped && stopped[0])) *out = (O)maxabs(acc[0].lo, acc[0].hi);
	}
};

// ---- host side: the grid (x: blocks, y: components) and the partials' storage are the caller's, (grid.y * K * grid.x elements) ----
template <class F, int K, class Term>
int reduce_partials(int64_t n, dim3 grid, Term term, typename F::T* partials, hipStream_t st) {
	hipLaunchKernelGGL((k_reduce_partials<F, K, Term>), grid, dim3(BLOCK), 0, st, n, term, partials);
	MF_LAUNCH_CHECK();
	return 0;
}
template <class F, int K, class Epi>
int reduce_finish(int nb, int ncomp, const typename F::T* partials, Epi epi, hipStream_t st) {
	hipLaunchKernelGGL((k_reduce_finish<F, K, Epi>), dim3(ncomp), dim3(BLOCK), 0, st, nb, partials, epi);
	MF_LAUNCH_CHECK();
	return 0;
}
template <class F, int K, class Term, class Epi>
int reduce(int64_t n, dim3 grid, Term term, typename F::T* partials, Epi epi, hipStream_t st) {
	MF_TRY((reduce_partials<F, K>(n, grid, term, partials, st)));
	return reduce_finish<F, K>((int)grid.x, (int)grid.y, partials, epi, st);
}

// the terms more than one file sums: fp32 products a * b accumulated in fp64 (GridDotProduct, conjugategrad.cpp:175-178)
struct DotTerm {
	const float *a, *b;
	__device__ __forceinline__ void operator()(int64_t i, double (&acc)[1]) const {
		const float pr = a[i] * b[i];
		acc[0] += (double)pr;
	}
};

}  // namespace mf
