/*
 * manta_hip_mesh.h -- C ABI extension of `libmanta_hip.so`: surface meshes.
 *   LevelsetGrid::createMesh   source/levelset.cpp:330-415 (marching cubes on the 1e-4 iso-surface of -phi)
 *   Mesh::advectInGrid         source/mesh.cpp:301-315 with integratePointSet, source/util/integrator.h:26-78
 *   Mesh::scale / offset / rotate   source/mesh.cpp:332-373
 * The mesh lives in caller-owned device arrays: nodes as pos[3][ncap], normal[3][ncap], flags[ncap]; triangles as c[3][tcap] (int32 node
 * numbers) and flags[tcap].  Saving, loading and computeVertexNormals are host code of the package and have no entry here.
 *
 * The rules are those of the other extension headers: include/manta_hip.h and MF_ABI_VERSION stay as they are; a library implements
 * the whole extension, reporting MF_MESH_ABI_VERSION through mf_mesh_abi_version(), or none of it.  Conventions (error plumbing, borrowed
 * device pointers, SoA, idx = i + sx*(j + sy*k), streams) are those of include/manta_hip.h.  The grid entries refuse a z-slab window
 * (mf_set_slab_window): grids are whole domains.  DESIGN.md section 16 has the contract of createMesh and the fp32 / fp64 map.
 */
#ifndef MANTA_HIP_MESH_H
#define MANTA_HIP_MESH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_mesh_scan_bytes, mf_mesh_create_plan, mf_mesh_create_emit, mf_mesh_advect, mf_mesh_scale, mf_mesh_offset, mf_mesh_rotate_pair,
 *      mf_mesh_sincos */
#define MF_MESH_ABI_VERSION 1
int mf_mesh_abi_version(void);

/* createMesh is two calls around the one read-back that sizes the mesh.  A cell is (i, j, k) with i < sx-1, j < sy-1, k < sz-1; its 8
 * corner values are -phi in the order (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1); bit l of its cube index is set
 * when -phi_l < 1e-4f.  A cell is inactive if a corner has phi <= -1000 or its cube index is 0 or 255.  An edge of an active cell is
 * crossed iff its two corner bits differ; its owner is the first active cell, in the sweep order k outer, j, i inner, of the up to four
 * cells that share it.  Node number = (exclusive scan, in sweep order, of the edges each cell owns) + (the owner's owned edges with a
 * smaller local edge number).  Triangles are numbered by the exclusive scan of the per-cell triangle counts and listed within a cell in
 * the order of the classic marching-cubes table.  Every dimension must be at least 3 (getGradient's clamp). */

/* *bytes_host = the size of `tmp` that mf_mesh_create_plan needs for this grid.  Touches no device memory. */
int mf_mesh_scan_bytes(int sx, int sy, int sz, int64_t* bytes_host);

/* classify, count, scan: cube[n] bytes (the cube index, 0 for an inactive cell and for the cells of the last row / column / plane),
 * mask[n] 16-bit words (the owned edges), nodeOff[n] and triOff[n] (the two exclusive scans), all written in full; tmp is scratch of
 * tmp_bytes >= mf_mesh_scan_bytes.  totals_host[0..1] = number of nodes, number of triangles.  Synchronises the stream: this 16-byte
 * read-back is the only one of createMesh. */
int mf_mesh_create_plan(int sx, int sy, int sz, const float* phi, void* cube, void* mask, int32_t* nodeOff, int32_t* triOff, void* tmp,
                        int64_t tmp_bytes, int64_t* totals_host, void* stream);

/* emit: the owner of each crossed edge writes its node -- with the orientation e1 -> e2 of its own local edge number,
 * mu = (1e-4f - v[e1]) / (v[e2] - v[e1]), pos = p1 + (p2 - p1) * mu + 0.5, normal = getNormalized(getGradient(e1 corner) * (1.0 - mu) +
 * getGradient(e2 corner) * mu) where the first factor is a double (each product rounded once) and the second a float; node flags 0 --
 * and every active cell writes its triangles (flags 0), looking its corner nodes up through the owners.  nNodes / nTris are the totals of
 * the plan; ncap >= nNodes and tcap >= nTris are the strides of the mesh arrays.  Asynchronous. */
int mf_mesh_create_emit(int sx, int sy, int sz, const float* phi, const void* cube, const void* mask, const int32_t* nodeOff,
                        const int32_t* triOff, int64_t nNodes, int64_t nTris, int64_t ncap, float* pos, float* normal, int32_t* nflags,
                        int64_t tcap, int32_t* tri, int32_t* tflags, void* stream);

/* Mesh::advectInGrid, one kernel: u = 0 for nodes with flag NfFixed (1) and for nodes outside isInBounds(pos, 1), else
 * vel.getInterpolated(pos) * dt; integrationMode 0 Euler, 1 RK2, 2 RK4 exactly as integratePointSet writes them (RK4 with the fork's
 * `uTotal += u`).  No clamp, no obstacle test, no delete: that is the difference from mf_advect_in_grid. */
int mf_mesh_advect(int sx, int sy, int sz, const float* vel, int64_t n, int64_t ncap, float* pos, const int32_t* nflags, float dt,
                   int integrationMode, void* stream);

/* pos *= s ; pos += o (component-wise, fp32) */
int mf_mesh_scale(int64_t n, int64_t ncap, float* pos, float x, float y, float z, void* stream);
int mf_mesh_offset(int64_t n, int64_t ncap, float* pos, float x, float y, float z, void* stream);

/* one axis pair of Mesh::rotate: a = pos[first], b = pos[second]; pos[first] = a * cos_t - b * sin_t, pos[second] = b * cos_t + a * sin_t
 * in fp32 without contraction.  The caller has the scalars from mf_mesh_sincos and has negated sin_t for the pair (0, 2). */
int mf_mesh_rotate_pair(int64_t n, int64_t ncap, float* pos, int first, int second, float sin_t, float cos_t, void* stream);

/* HOST entry: *sin_host = sinf(theta), *cos_host = cosf(theta) with the C library's float functions (what `sin(Real)` resolves to in
 * mesh.cpp).  Touches no device. */
int mf_mesh_sincos(float theta, float* sin_host, float* cos_host);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_MESH_H */
