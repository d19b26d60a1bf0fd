/*
 * manta_hip_mlflip.h -- C ABI extension of `libmanta_hip.so`: the array bridge and the MLFLIP data plugins.
 *   copyArrayToGrid* / copyGridToArray* / copyArrayToPdata* / copyPdataToArray*    source/plugin/numpyconvert.cpp:29-223
 *   simpleNumpyTest, extractFeatureVel / Phi / Geo                                  source/plugin/tfplugins.cpp:22-148
 *   getRegions, getRegionalCounts, extendRegion, markSmallRegions                   source/plugin/tfplugins.cpp:155-220
 * An "array" is caller-owned DEVICE memory in the element-major layout of numpy: [z][y][x] for a scalar grid, [z][y][x][3] for a
 * vector grid, [i] / [i][3] for particle data.  Grids and Vec3 channels are component planes (data[c * n + idx], pd[c * cap + i]), so
 * the vector copies transpose.  The host layer stages host arrays; nothing here touches host memory except the one count that
 * mf_mlflip_regions reads back.
 *
 * The rules are those of the other extension headers: include/manta_hip.h and MF_ABI_VERSION stay as they are; a library implements
 * the whole extension, reporting MF_MLFLIP_ABI_VERSION through mf_mlflip_abi_version(), or none of it.  Conventions (error plumbing,
 * borrowed device pointers, idx = i + sx*(j + sy*k), streams) are those of include/manta_hip.h.  Every grid entry refuses a z-slab
 * window.  DESIGN.md section 22 has the kernel forms.
 */
#ifndef MANTA_HIP_MLFLIP_H
#define MANTA_HIP_MLFLIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_mlflip_convert, mf_mlflip_planes_to_elements, mf_mlflip_elements_to_planes, mf_mlflip_extract_feature,
 *      mf_mlflip_regions, mf_mlflip_extend_region, mf_mlflip_mark_small_regions, mf_mlflip_simple_array_add */
#define MF_MLFLIP_ABI_VERSION 1
int mf_mlflip_abi_version(void);

/* element types of an array or a grid */
#define MF_MLFLIP_INT32 0
#define MF_MLFLIP_FLOAT32 1
#define MF_MLFLIP_FLOAT64 2

/* dst[q] = (dst type)src[q] for q < n: the C conversion of the reference's assignments (float / double to int truncates towards zero,
 * double to float and int to float round to nearest).  Equal types are one device-to-device memcpy.  Both are device memory of their
 * type's alignment and do not overlap.  Asynchronous. */
int mf_mlflip_convert(int64_t n, const void* src, int src_type, void* dst, int dst_type, void* stream);

/* The vector copies: arr[q * 3 + c] = (array type)planes[c * stride + q] for q < n, c < 3, and the other direction.  planes is fp32
 * (a Vec3 / MAC grid with stride == n, a Vec3 particle channel with stride == cap >= n); arr_type is FLOAT32 or FLOAT64.  One kernel,
 * one thread per element q: the element-major side moves as one 12-byte (24-byte) access per lane, contiguous over the wave; every
 * access is non-temporal.  Asynchronous. */
int mf_mlflip_planes_to_elements(int64_t n, int64_t stride, const float* planes, void* arr, int arr_type, void* stream);
int mf_mlflip_elements_to_planes(int64_t n, int64_t stride, const void* arr, int arr_type, float* planes, void* stream);

/* extractFeatureVel (kind 0: grid is a MAC grid, D = 3 values per stencil point, 2 on a 2-D grid), extractFeaturePhi (kind 1: a Real
 * grid, D = 1) and extractFeatureGeo (kind 2: a flag grid, D = 1).  For every slot p < np whose pflag has no PDELETE (1 << 10) and
 * whose ptype (nullable) has no bit of `exclude`, and every stencil point s = ((i + window) * W + (j + window)) * Wk + (k + window)
 * with W = 2 * window + 1, Wk = W in 3-D and 1 (k = 0) in 2-D:
 *   fv[p * N_row + off_begin + s * D + c] = value_c(pos[p] + (i, j, k)) * scale        (the sum and the product in fp32)
 * value = interpolMAC, interpol, or float(flags at the cell the position truncates to; the cell index is clamped into the grid).
 * Nothing else of fv (fv_len floats) is written.  One thread per (p, s), s fastest.
 * Refused: np < 0, cap < np, window < 0, off_begin < 0, off_begin + nStencil * D > N_row, fv_len < np * N_row.  Asynchronous. */
int mf_mlflip_extract_feature(int kind, int sx, int sy, int sz, const void* grid, int64_t np, int64_t cap, const float* pos,
                              const int32_t* pflag, const int32_t* ptype, int exclude, int window, float scale, float* fv, int64_t fv_len,
                              int64_t N_row, int64_t off_begin, void* stream);

/* Connected components of the cells with flags & ctype, face neighbours inside the grid only (6 in 3-D, 4 in 2-D).
 *   counts == 0 (getRegions):        r = 0 outside, else 1 + the rank of the component among all components ordered by their lowest
 *                                    flat index; *count_host = the number of components (the one value read back; synchronises)
 *   counts != 0 (getRegionalCounts): r = 0 outside, else the number of cells of the component; count_host is not written and nothing
 *                                    is read back
 * Union-find over the flat index with 32-bit atomicMin on the roots, so a component's root is its lowest index whatever order the
 * atomics land in; scratch comes from the per-device arena. */
int mf_mlflip_regions(int sx, int sy, int sz, const int32_t* flags, int ctype, int counts, int32_t* r, int32_t* count_host, void* stream);

/* extendRegion: `depth` rounds; in a round every cell without flags & exclude that has a face neighbour inside the grid with
 * flags & region becomes exactly `region`, all cells decided from the flags before the round.  tmp is a scratch grid of the same
 * size; the result is in flags.  depth <= 0: nothing.  Asynchronous. */
int mf_mlflip_extend_region(int sx, int sy, int sz, int32_t* flags, int32_t* tmp, int region, int exclude, int depth, void* stream);

/* markSmallRegions: flags = mark where !(flags & exclude) and rcnt <= th.  Asynchronous. */
int mf_mlflip_mark_small_regions(int sx, int sy, int sz, int32_t* flags, const int32_t* rcnt, int mark, int exclude, int th, void* stream);

/* simpleNumpyTest: grid(i, j, k) += scale * arr[j * sx + i] for every k; arr holds arr_len >= sx * sy floats.  Asynchronous. */
int mf_mlflip_simple_array_add(int sx, int sy, int sz, float* grid, const float* arr, int64_t arr_len, float scale, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_MLFLIP_H */
