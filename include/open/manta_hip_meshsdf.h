/*
 * manta_hip_meshsdf.h -- C ABI extension of `libmanta_hip.so`: mesh-to-level-set rasterisation.
 *   meshSDF                    source/mesh.cpp:868-1005 with SDFKernel :769-820 and _cIndex :822-826
 *   ApplyMeshToGrid            source/mesh.cpp:829-837
 *   KnApplyDensity             source/plugin/initplugins.cpp:132-137
 * meshSDF is five calls: plan (count + scan, one read-back that sizes the source buffers), emit, bin, gather, flood.  The mesh is read
 * from the arrays of include/open/manta_hip_mesh.h (pos[3][ncap], c[3][tcap]); sources are pos[3][scap] / normal[3][scap].
 *
 * The rules are those of the other extension headers: include/manta_hip.h and MF_ABI_VERSION stay as they are; a library implements
 * the whole extension, reporting MF_MESHSDF_ABI_VERSION through mf_meshsdf_abi_version(), or none of it.  Conventions (error plumbing,
 * borrowed device pointers, SoA, idx = i + sx*(j + sy*k), streams) are those of include/manta_hip.h.  Every grid entry needs a 3-D grid
 * and refuses a z-slab window (mf_set_slab_window).  DESIGN.md section 17 has the contract of each stage and the fp32 / fp64 map.
 */
#ifndef MANTA_HIP_MESHSDF_H
#define MANTA_HIP_MESHSDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_meshsdf_tmp_bytes, mf_meshsdf_plan, mf_meshsdf_emit, mf_meshsdf_bin, mf_meshsdf_gather, mf_meshsdf_flood, mf_meshsdf_apply,
 *      mf_meshsdf_apply_density */
#define MF_MESHSDF_ABI_VERSION 1
int mf_meshsdf_abi_version(void);

/* *bytes_host = the size of `tmp` that serves mf_meshsdf_plan for nTris triangles and mf_meshsdf_bin for nSrc sources on nCells cells.
 * Touches no device memory. */
int mf_meshsdf_tmp_bytes(int64_t nTris, int64_t nSrc, int64_t nCells, int64_t* bytes_host);

/* Sources, count and scan.  Triangle t yields its face centre and, if an edge is longer than 0.75 (norm of getEdge in mesh units),
 * the barycentric samples (s0, s1), s0 < iterA outer, s1 < iterB inner, with w = 1 - u - v >= 0 where u = (float)((double)s0 / iterA),
 * v = (float)((double)s1 / iterB) and w is fp32; (pointA, pointB, iterA, iterB) follow the three branches of mesh.cpp:898-919 with
 * numSamplesN = (short)(int)(norm(edge) * 0.75f).  off[nTris] (int64) = the exclusive scan of the per-triangle counts, *total_host = their
 * sum.  Fails, naming the cause, when a triangle names a node outside [0, nNodes) or a sample count does not fit the reference's
 * `short` (an edge of 43 690 units or more), or when the total does not fit 31 bits.  Synchronises the stream: this read-back is the
 * one that sizes the source buffers. */
int mf_meshsdf_plan(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, int64_t* off, void* tmp,
                    int64_t tmp_bytes, int64_t* total_host, void* stream);

/* Sources, emit: spos / snrm [3][scap], entries off[t] ... of triangle t: ((p0 + p1) + p2) / 3.0 (double quotient, rounded once) times
 * mult, then the samples ((pA * mult) * u + (pB * mult) * v) + (pC * mult) * w per component in fp32 without contraction; every source of a
 * triangle carries getNormalized(cross(p1 - p0, p2 - p0)).  total is the plan's; scap >= total.  Asynchronous. */
int mf_meshsdf_emit(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, const int64_t* off,
                    int64_t total, float mx, float my, float mz, int64_t scap, float* spos, float* snrm, void* stream);

/* Binning: the cell of a source is ((int)x, (int)y, (int)z) -- truncation toward zero first, then the bounds test, so a coordinate in
 * (-1, 0) lands in cell 0; sources outside are dropped.  len[n] / start[n] = sources per cell and their exclusive scan in cell-index
 * order; bpos / bnrm [3][scap] = the sources sorted by cell, source order kept within a cell; occ = one int per 8x8x8 block of cells
 * (x fastest, ceil(sx/8) * ceil(sy/8) * ceil(sz/8) of them), non-zero where the block holds a source.  keys = 4 * scap ints of scratch.
 * stats[0] (device) = number of sources binned.  Asynchronous. */
int mf_meshsdf_bin(int sx, int sy, int sz, int64_t nSrc, int64_t scap, const float* spos, const float* snrm, int32_t* keys, float* bpos,
                   float* bnrm, int32_t* len, int32_t* start, int32_t* occ, int32_t* stats, void* tmp, int64_t tmp_bytes, void* stream);

/* Gather, one thread per cell, every cell written: with c = cutoff < 0 ? 2 * sigma : cutoff (fp32), safeRadius = (float)(c + sqrt(3.0) *
 * 0.5), isigma2 = (float)(1.0 / (double)(sigma * sigma)), intRadius = (int)(c + 0.5): over the block [cell - intRadius, cell + intRadius]
 * clamped to the grid, i outer, j, k inner, skipping cells with |d|^2 > safeRadius^2, over the cell's sources in binned order:
 * r = (cell + 0.5) - pos, r2 = |r|^2; if r2 < c^2: w = (float)exp((double)(-r2 * isigma2)), sum += w, dist += dot(normal, r) * w (fp32,
 * no contraction).  phi = sum > 0 ? dist / sum : -c.  A cell whose block meets no occupied 8x8x8 block skips the visit.  sigma > 0. */
int mf_meshsdf_gather(int sx, int sy, int sz, int64_t scap, const float* bpos, const float* bnrm, const int32_t* len, const int32_t* start,
                      const int32_t* occ, float sigma, float cutoff, float* phi, void* stream);

/* Flood fill of the outside: cells with phi >= c - 1.0f are seeds; every seed, and every cell reachable from a seed through 6-neighbours
 * whose value is < 0, takes the value c (the end state of the reference's stack loop, for c >= 0).  Fixed point inside 8x8x8 tiles in
 * LDS, one launch per round until a launch changes nothing; one int is read back per round.  stats (device, 4 ints) is scratch whose
 * entry 0 is mf_meshsdf_bin's; out_host[0] = rounds launched (the last one changed nothing), out_host[1] = stats[0].  With flood == 0
 * nothing is filled (the field stays as the gather left it) and only out_host[1] is read.  Synchronises the stream. */
int mf_meshsdf_flood(int sx, int sy, int sz, float* phi, float sigma, float cutoff, int flood, int32_t* stats, int32_t* out_host, void* stream);

/* ApplyMeshToGrid: cells with sdf < 0 that are not obstacles of `flags` (nullable) take the value.  kind 0: int grid <- ivalue; 1: real
 * grid <- vx; 2: Vec3 / MAC grid (SoA planes) <- (vx, vy, vz). */
int mf_meshsdf_apply(int sx, int sy, int sz, const float* sdf, const int32_t* flags, int kind, void* grid, int ivalue, float vx, float vy,
                     float vz, void* stream);

/* KnApplyDensity: fluid cells with sdf <= sigma take `value`. */
int mf_meshsdf_apply_density(int sx, int sy, int sz, const int32_t* flags, float* density, const float* sdf, float value, float sigma,
                             void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_MESHSDF_H */
