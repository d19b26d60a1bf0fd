/*
 * manta_hip_meshops.h -- C ABI extension of `libmanta_hip.so`: mesh connectivity and smoothing.
 *   Mesh::rebuildCorners / rebuildLookup   source/mesh.cpp:238-292 (the corner table's `opposite`, the 1-ring lookup)
 *   Mesh::computeCenterOfMass              source/mesh.cpp:123-141
 *   smoothMesh                             source/plugin/meshplugins.cpp:36-104
 * The mesh is read from the arrays of include/open/manta_hip_mesh.h (pos[3][ncap], flags[ncap], c[3][tcap]).
 *
 * The rules are those of the other extension headers: include/manta_hip.h and MF_ABI_VERSION stay as they are; a library implements
 * the whole extension, reporting MF_MESHOPS_ABI_VERSION through mf_meshops_abi_version(), or none of it.  Conventions (error plumbing,
 * borrowed device pointers, SoA, streams) are those of include/manta_hip.h.  Every device entry refuses a z-slab window
 * (mf_set_slab_window).  DESIGN.md section 26 has the group rule of the corner table, the fp32 / fp64 map and the reduction bound.
 */
#ifndef MANTA_HIP_MESHOPS_H
#define MANTA_HIP_MESHOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_meshops_tmp_bytes, mf_meshops_build, mf_meshops_smooth_step, mf_meshops_volume_terms, mf_meshops_volume_sums,
 *      mf_meshops_rescale_scalars, mf_meshops_rescale, mf_meshops_kill_plan, mf_meshops_kill_apply */
#define MF_MESHOPS_ABI_VERSION 1
int mf_meshops_abi_version(void);

/* *bytes_host = the size of `tmp` that serves mf_meshops_build, mf_meshops_volume_sums and the two mf_meshops_kill_* entries for a mesh of nTris triangles and nNodes
 * nodes.  Touches no device memory. */
int mf_meshops_tmp_bytes(int64_t nTris, int64_t nNodes, int64_t* bytes_host);

/* The connectivity tables, a pure function of the triangle list.
 *   opposite[3 * nTris]: corner 3t + k has node c[k][t], next 3t + (k + 1) % 3 and prev 3t + (k + 2) % 3; its key is the unordered pair
 *     of its next and prev nodes.  Within the corners c_1 < ... < c_g of one key, opposite[c_i] = c_{i+1} for i < g and
 *     opposite[c_g] = c_{g-1}: what the forward search of mesh.cpp:256-271 leaves.  A key with one corner gets -1.
 *   nodeOff[nNodes + 1], ringNodes[<= 6 * nTris]: per node the ascending, duplicate-free next and prev nodes of its corners (CSR).
 *   triOff[nNodes + 1], ringTris[3 * nTris]: per node its triangles, ascending (CSR).
 * Stable radix sorts of the 3 * nTris corners and the 6 * nTris (node, neighbour) pairs, one pass over each sorted array, one 16-byte
 * read-back: out_host[0] = keys with one corner, [1] = keys with three or more, [2] = the first triangle with a repeated node, [3] = the
 * first triangle that names a node outside [0, nNodes) (-1: none).  When [2] or [3] is set the tables are not written (the offsets are
 * zero).  Synchronises the stream. */
int mf_meshops_build(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int32_t* opposite, int32_t* nodeOff, int32_t* ringNodes,
                     int32_t* triOff, int32_t* ringTris, void* tmp, int64_t tmp_bytes, int32_t* out_host, void* stream);

/* One Jacobi step of smoothMesh, one lane per node, into temp[3][nNodes] and back to the nodes without NfFixed (1).  A node without a
 * triangle gets (0, 0, 0).  Otherwise, over its ring in ascending order: edge = pos_j - pos (fp32), len = norm(edge) (vectorbase.h:384);
 * while len > minLength: dx += (float)((double)edge * (1.0 / (double)len)) per component, totalLen += len; the first len <= minLength
 * sets totalLen = 0 and ends the walk.  temp = pos, and if totalLen != 0, temp += dx * (str / totalLen) in fp32.  No contraction. */
int mf_meshops_smooth_step(int64_t nNodes, int64_t ncap, float* pos, const int32_t* nflags, const int32_t* nodeOff, const int32_t* ringNodes,
                           const int32_t* triOff, float str, float minLength, float* temp, void* stream);

/* terms[4][nTris] (fp64) of Mesh::computeCenterOfMass: cvol = dot(cross(p1, p2), p3) / 6.0 and ((p1 + p2) + p3) * (cvol / 4.0) per
 * component, all in double from the float positions, no contraction.  The triangles must name nodes inside the mesh. */
int mf_meshops_volume_terms(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, double* terms,
                            void* stream);

/* sums_host[4] = the sums of those terms over the triangles in a fixed tree (256 consecutive triangles per block by shuffles, then
 * one block over the partials): the same bits from run to run, and within 2 * gamma_{nTris-1} * sum|term| of the serial sum.
 * Synchronises the stream (one 32-byte read-back). */
int mf_meshops_volume_sums(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, void* tmp,
                           int64_t tmp_bytes, double* sums_host, void* stream);

/* Host: from the sums before and after the steps, out_host[0..2] = origCM, [3..5] = newCM (sums[1..3] / sums[0] where sums[0] != 0,
 * rounded to float), [6] = beta = cbrtf((float)sums0[0] / (float)sums1[0]) -- `cbrt(Real / Real)` of meshplugins.cpp:98 resolves to
 * the float overload.  A zero new volume gives inf / nan, as in the reference. */
int mf_meshops_rescale_scalars(const double* sums0_host, const double* sums1_host, float* out_host);

/* pos = origCM + (pos - newCM) * beta (fp32) on the nodes without NfFixed. */
int mf_meshops_rescale(int64_t nNodes, int64_t ncap, float* pos, const int32_t* nflags, float ox, float oy, float oz, float nx, float ny, float nz,
                       float beta, void* stream);

/* killSmallComponents, the plan: nothing of the mesh is written.  `opposite` is mf_meshops_build's table of this triangle list, with no
 * key of one corner and none of three or more.  Components of the triangle graph t -- opposite[3t + c] / 3 are labelled with their
 * smallest triangle by rounds of hooking to the smaller label and pointer jumping (one int read back per round); a triangle is tainted
 * when its component has fewer than `elements` triangles.  Left in `tmp` for mf_meshops_kill_apply: the taint mask and its exclusive
 * scan, per node the first tainted corner that names it, and deletedNodes -- the nodes of the tainted triangles in the order of that
 * first corner (triangles ascending, corners 0..2).  out_host[0] = rounds (the last one changed nothing), [1] = components, [2] = tainted
 * triangles, [3] = deleted nodes, [4] = the smallest deleted node that a kept triangle names as well (-1: none; the caller refuses the
 * mesh then).  Synchronises the stream. */
int mf_meshops_kill_plan(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, const int32_t* opposite, int elements, void* tmp,
                         int64_t tmp_bytes, int32_t* out_host, void* stream);

/* killSmallComponents, the removal, with the plan's `tmp` untouched in between and its two counts.  Triangles: removeTri (mesh.cpp:401-448)
 * over the tainted triangles in descending order -- each takes the then-last triangle with its flags -- as one pass: with below[q] the
 * tainted triangles < q, the kept slot h (tainted, h < nTris - killedTris) receives the triangle at the end of the chain
 * q <- nTris - (killedTris - below[q]), started at h and followed while q is tainted.  Nodes: removeNodes (mesh.cpp:450-508) with
 * newsize = nNodes - deletedNodes: the i-th node >= newsize that is not deleted (ascending) moves, with position, normal and flags, to
 * the i-th entry of deletedNodes (list order) that is < newsize, and the triangles are renumbered.  The mesh then has
 * nTris - killedTris triangles and nNodes - deletedNodes nodes.  Asynchronous. */
int mf_meshops_kill_apply(int64_t nTris, int64_t tcap, int32_t* tri, int32_t* tflags, int64_t nNodes, int64_t ncap, float* pos, float* normal,
                          int32_t* nflags, int64_t killedTris, int64_t deletedNodes, void* tmp, int64_t tmp_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_MESHOPS_H */
