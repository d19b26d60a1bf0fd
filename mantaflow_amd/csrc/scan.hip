// scan.hip -- hipcub's DeviceScan / DeviceRadixSort behind plain functions (scan.h): the one translation unit that pays for the
// library's templates, and the one instantiation of each primitive the extensions share.
#include "scan.h"
#include <hipcub/hipcub.hpp>

namespace mf {

// every caller's n is below 2^31 (check_dim, the particle-count checks), so the cap at 31 never binds; it keeps the sign bit of an
// int32_t key out of the sorted range whatever n is
int key_bits(int64_t n) {
	int b = 1;
	while (b < 31 && ((int64_t)1 << b) <= n) b++;
	return b;
}

// hipcub's own size query: the call with no workspace writes the size and launches nothing.  What it wrote counts even where it
// then reports an error (no device), so that the scratch-size entries answer the same with and without a GPU
template <class F>
static int raise_to(size_t* bytes, F query) {
	size_t q = 0;
	const hipError_t e = query(q);
	if (q > *bytes) *bytes = q;
	MF_HIP(e);
	return 0;
}
int exclusive_sum32_bytes(int64_t n, size_t* bytes) {
	return raise_to(bytes, [n](size_t& q) { return hipcub::DeviceScan::ExclusiveSum(nullptr, q, (int32_t*)nullptr, (int32_t*)nullptr, (int)n, (hipStream_t)0); });
}
int exclusive_sum64_bytes(int64_t n, size_t* bytes) {
	return raise_to(bytes, [n](size_t& q) { return hipcub::DeviceScan::ExclusiveSum(nullptr, q, (int64_t*)nullptr, (int64_t*)nullptr, (int)n, (hipStream_t)0); });
}
int inclusive_sum32_bytes(int64_t n, size_t* bytes) {
	return raise_to(bytes, [n](size_t& q) { return hipcub::DeviceScan::InclusiveSum(nullptr, q, (int32_t*)nullptr, (int32_t*)nullptr, (int)n, (hipStream_t)0); });
}
int sort_pairs_bytes(int64_t n, int bits, size_t* bytes) {
	return raise_to(bytes, [n, bits](size_t& q) {
		return hipcub::DeviceRadixSort::SortPairs(nullptr, q, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (int)n, 0, bits, (hipStream_t)0);
	});
}

int exclusive_sum(void* ws, size_t ws_bytes, int32_t* in, int32_t* out, int64_t n, hipStream_t st) { MF_HIP(hipcub::DeviceScan::ExclusiveSum(ws, ws_bytes, in, out, (int)n, st)); return 0; }
int exclusive_sum(void* ws, size_t ws_bytes, int64_t* in, int64_t* out, int64_t n, hipStream_t st) { MF_HIP(hipcub::DeviceScan::ExclusiveSum(ws, ws_bytes, in, out, (int)n, st)); return 0; }
int inclusive_sum(void* ws, size_t ws_bytes, int32_t* in, int32_t* out, int64_t n, hipStream_t st) { MF_HIP(hipcub::DeviceScan::InclusiveSum(ws, ws_bytes, in, out, (int)n, st)); return 0; }
int sort_pairs(void* ws, size_t ws_bytes, uint32_t* keys_in, uint32_t* keys_out, int32_t* vals_in, int32_t* vals_out, int64_t n,
               int bits, hipStream_t st) {
	MF_HIP(hipcub::DeviceRadixSort::SortPairs(ws, ws_bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, bits, st));
	return 0;
}

}  // namespace mf
