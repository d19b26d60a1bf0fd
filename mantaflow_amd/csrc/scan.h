// scan.h -- the device-wide prefix sums and the radix sort the extensions use; scan.hip alone includes the library behind them.
// Every function returns the library's error convention.
#pragma once
#include "common.h"

namespace mf {

// width of the keys 0 .. n (cell indices, n itself for "no cell"): the sorts look at bits [0, key_bits(n)) only
int key_bits(int64_t n);

// raise *bytes to the workspace that the call of the same name needs for n elements: after the queries of all its calls, *bytes is
// the size of the one workspace an entry point shares among them
int exclusive_sum32_bytes(int64_t n, size_t* bytes);
int exclusive_sum64_bytes(int64_t n, size_t* bytes);
int inclusive_sum32_bytes(int64_t n, size_t* bytes);
int sort_pairs_bytes(int64_t n, int bits, size_t* bytes);

// the calls, on the stream, with a workspace of at least the queried size; a scan may run in place (in == out).  The inputs are
// plain pointers so that each primitive has the one instantiation (and kernel name) it had inside the extensions
int exclusive_sum(void* ws, size_t ws_bytes, int32_t* in, int32_t* out, int64_t n, hipStream_t st);
int exclusive_sum(void* ws, size_t ws_bytes, int64_t* in, int64_t* out, int64_t n, hipStream_t st);
int inclusive_sum(void* ws, size_t ws_bytes, int32_t* in, int32_t* out, int64_t n, hipStream_t st);
// stable, 32-bit keys with int32_t values.  The keys are unsigned: every caller's are non-negative, so int32_t keys (cast at the
// call) sort the same
int sort_pairs(void* ws, size_t ws_bytes, uint32_t* keys_in, uint32_t* keys_out, int32_t* vals_in, int32_t* vals_out, int64_t n,
               int bits, hipStream_t st);

}  // namespace mf
