/*
 * manta_hip_vsheet.h -- C ABI extension of `libmanta_hip.so`: vortex sheets.
 *   VortexSheetMesh::calcVorticity / reinitTexCoords   source/vortexsheet.cpp:45-59, 78-91
 *   texcoordInflow, meshSmokeInflow                    source/plugin/vortexplugins.cpp:41-75
 *   vorticitySource, smoothVorticity                   source/plugin/vortexplugins.cpp:77-166
 *   VICintegration                                     source/plugin/vortexplugins.cpp:192-295
 * The mesh is read from the arrays of include/open/manta_hip_mesh.h (pos[3][ncap], flags[ncap], c[3][tcap]); the sheet's channels are
 * planes of the same strides: per triangle vorticity, vorticitySmoothed, circulation ([3][tcap] each), smokeAmount, smokeParticles
 * ([tcap] each); per node tex1, tex2 ([3][ncap] each).  The per-triangle geometry (getFaceCenter, getFaceArea, getFaceNormal, getEdge,
 * isTriangleFixed, source/mesh.h:207-215) is inlined into the kernels.
 *
 * The rules are those of the other extension headers: include/manta_hip.h and MF_ABI_VERSION stay as they are; a library implements
 * the whole extension, reporting MF_VSHEET_ABI_VERSION through mf_vsheet_abi_version(), or none of it.  Conventions (error plumbing,
 * borrowed device pointers, SoA, streams) are those of include/manta_hip.h.  Every device entry refuses a z-slab window
 * (mf_set_slab_window).  A triangle that names a node outside [0, nNodes) is skipped by every entry.  A shape travels as (kind,
 * 12 floats), the record of mf_shape_levelset.  DESIGN.md section 28 has the fp32 / fp64 map and the bound of the one transcendental.
 */
#ifndef MANTA_HIP_VSHEET_H
#define MANTA_HIP_VSHEET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_vsheet_calc_vorticity, mf_vsheet_reinit_tex, mf_vsheet_smoke_inflow, mf_vsheet_acceleration, mf_vsheet_source,
 *      mf_vsheet_smooth_weights, mf_vsheet_smooth_iterate, mf_vsheet_inflow_tmp_bytes, mf_vsheet_inflow_mean,
 *      mf_vsheet_inflow_apply, mf_vsheet_spread_tmp_bytes, mf_vsheet_spread, mf_vsheet_curl, mf_vsheet_rhs, mf_vsheet_set_component */
#define MF_VSHEET_ABI_VERSION 1
int mf_vsheet_abi_version(void);

/* VortexSheetMesh::calcVorticity, vortexsheet.cpp:45-59, one thread per triangle: smokeAmount = 0; vorticity = 0 where
 * (double)getFaceArea < 1e-10, else (circulation[0] * e0 + circulation[1] * e1 + circulation[2] * e2) / area in fp32, left to right, with
 * e_k = getEdge(t, k).  Asynchronous. */
int mf_vsheet_calc_vorticity(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, const float* circulation,
                             float* vorticity, float* smokeAmount, void* stream);

/* VortexSheetMesh::reinitTexCoords, vortexsheet.cpp:78-91, one thread per node: tex1 = tex2 = pos + mTexOffset.  Asynchronous. */
int mf_vsheet_reinit_tex(int64_t nNodes, int64_t ncap, const float* pos, float ox, float oy, float oz, float* tex1, float* tex2, void* stream);

/* meshSmokeInflow, vortexplugins.cpp:69-75, one thread per triangle: smokeAmount = amount where the shape's isInside holds at
 * getFaceCenter -- ((p0 + p1) + p2 in fp32, each component then divided by 3.0 in double and rounded once).  Asynchronous. */
int mf_vsheet_smoke_inflow(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, int kind,
                           const float* params_host, float amount, float* smokeAmount, void* stream);

/* KnAcceleration, vortexplugins.cpp:77-80: accel = (v1 - v0) * idt over the three planes of a MAC grid, border included.  The caller
 * forms idt = (Real)(1.0 / dt).  Asynchronous. */
int mf_vsheet_acceleration(int sx, int sy, int sz, const float* v1, const float* v0, float idt, float* accel, void* stream);

/* vorticitySource, vortexplugins.cpp:95-117, one thread per triangle.  accel (nullable: no vel was given) is sampled with interpolMAC
 * at the face centre; source = (A * cross(getFaceNormal, a - gravity)) * scale with A = -1 (cross(fn, -gravity) without accel), zero on a
 * triangle with an NfFixed node; vorticity *= mult; vorticity += (dt * source) / dx; v = norm(vorticity); where maxAmount > 0 and
 * v > maxAmount, vorticity *= maxAmount / v.  norms[nTris] receives v.  stats_host[0] = max v (from 0, exact), [1] = the fp64 sum of v in
 * the fixed tree of the library's reductions (the reference prints sum / nTris of its serial fp32 sum).  3-D grids.  Synchronises the
 * stream (one 16-byte read-back). */
int mf_vsheet_source(int sx, int sy, int sz, const float* accel, int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap,
                     const float* pos, const int32_t* nflags, float gx, float gy, float gz, float scale, float maxAmount, float mult, float dt, float dx,
                     float* vorticity, float* norms, double* stats_host, void* stream);

/* smoothVorticity's table, vortexplugins.cpp:134-147, one thread per corner: with oc = opposite[3 i + c] (mf_meshops_build's table of
 * this triangle list) and t = oc / 3, weights[3 i + c] = exp(normSquare(centre_t - centre_i) * mult) and index[3 i + c] = t; weight 0 and
 * index 0 where oc < 0.  The reference's exp is the float overload; this is the fp64 exp of the widened fp32 argument, rounded once to
 * fp32: at most one fp32 unit in the last place from the reference.  The caller forms mult = (Real)(-0.5 / sigma / sigma).  Asynchronous. */
int mf_vsheet_smooth_weights(int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap, const float* pos, const int32_t* opposite,
                             float mult, float* weights, int32_t* index, void* stream);

/* smoothVorticity's passes, vortexplugins.cpp:149-165: from v = vorticity, `iter` Jacobi passes
 *   v_i <- (v_i + sum_c w_c * v[index[3 i + c]]) / (1 + sum_c w_c),  c = 0, 1, 2 in order,  w_c = weights[index[3 i + c]]
 * -- the weight is read at the neighbour triangle's NUMBER, as the reference's line 158 has it -- then smoothed = v * alpha.  vorticity is
 * not written.  A triangle whose index entries do not name triangles keeps its value in every pass.  tmp0, tmp1: [3][nTris] floats each.  Bit-identical to the reference given the table.  Asynchronous. */
int mf_vsheet_smooth_iterate(int64_t nTris, int64_t tcap, const float* weights, const int32_t* index, int iter, float alpha, const float* vorticity,
                             float* smoothed, float* tmp0, float* tmp1, void* stream);

/* *bytes_host = the size of `tmp` that serves mf_vsheet_inflow_mean on a grid of that size (vortexplugins.cpp:45-55).  Touches no device
 * memory. */
int mf_vsheet_inflow_tmp_bytes(int sx, int sy, int sz, int64_t* bytes_host);

/* texcoordInflow's mean, vortexplugins.cpp:45-55: the fp32 sum of MACGrid::getCentered over the cells whose centre is inside the shape,
 * added serially in the linear cell order (FOR_IJK: k outer, i inner); meanV = sum / (Real)cnt (NaN for cnt == 0);
 * out_host[0..2] = t0 - dt * meanV.  One thread per cell marks the inside cells, an inclusive scan ranks them, they write their samples
 * at their rank, and one wave adds that list in order, so the serial part costs what the inside cells cost.  out_host[3] != 0: an inside
 * cell lies in the last z plane, where getCentered reads outside the grid (such a cell is not read; the caller refuses the call).
 * mark: sx * sy * sz ints, values: 3 * sx * sy * sz floats, tmp: mf_vsheet_inflow_tmp_bytes.  3-D grids.  Synchronises the stream (one
 * 16-byte read-back). */
int mf_vsheet_inflow_mean(int sx, int sy, int sz, const float* vel, int kind, const float* params_host, float t0x, float t0y, float t0z, float dt,
                          int32_t* mark, float* values, void* tmp, int64_t tmp_bytes, float* out_host, void* stream);

/* texcoordInflow's nodes, vortexplugins.cpp:59-65, one thread per node: tex1 = tex2 = pos + t0 where isInside(pos).  Asynchronous. */
int mf_vsheet_inflow_apply(int64_t nNodes, int64_t ncap, const float* pos, int kind, const float* params_host, float t0x, float t0y, float t0z,
                           float* tex1, float* tex2, void* stream);

/* *bytes_host = the size of `tmp` that serves mf_vsheet_spread (vortexplugins.cpp:203-248) for that grid, sigma and triangle count.
 * Touches no device memory. */
int mf_vsheet_spread_tmp_bytes(int sx, int sy, int sz, float sigma, int64_t nTris, int64_t* bytes_host);

/* VICintegration's spreading, vortexplugins.cpp:203-248: vort[3][n] (every cell written) = per cell the fp32 sum of v_t * w over the
 * triangles that reach it, in ascending triangle number, with v_t = (vorticity * getFaceArea) * 16, sgi = ceil(sigma),
 * pkfac = (Real)(M_PI / sigma), the loops i, j, k in [-sgi, sgi), the skip tests `pos + i < 0` (float) and `(int)pos + i >= size`, the
 * cell the truncation of the float sum, flags.isFluid(cell), d = pos - (i + 0.5 + floor(pos)) formed in double and rounded, dl > sigma
 * skipped, w = (float)((1.0 + cos(dl * pkfac)) * wnorm), wnorm[t] = (float)(1.0 / sum) of the triangle's own stencil (pass A, one thread
 * per triangle, the sum in i, j, k order).  Pass B: the triangles are binned by the cell of their centre with a stable sort, and one
 * thread per cell merges the bins that can reach it by triangle number; no atomics.  cos is the fp64 function of the widened fp32
 * argument rounded once (the reference calls the float overload).  A float sum pos + i that rounds onto `size` addresses a cell
 * outside the grid in the reference; here that cell is left out (precondition: no such centre).  Asynchronous. */
int mf_vsheet_spread(int sx, int sy, int sz, const int32_t* flags, int64_t nTris, int64_t tcap, const int32_t* tri, int64_t nNodes, int64_t ncap,
                     const float* pos, const float* vorticity, float sigma, float* wnorm, float* vort, void* tmp, int64_t tmp_bytes, void* stream);

/* CurlOp of vortexplugins.cpp:267 (commonkernels.h:38-47, KERNEL(bnd=1)): curl[3][n] of the centred vort[3][n]; the border is zero. */
int mf_vsheet_curl(int sx, int sy, int sz, const float* vort, float* curl, void* stream);

/* the rhs of component c, vortexplugins.cpp:272-275: shifted != 0: GetShiftedComponent (0.5 * (g + g one cell down along c), bnd = 1:
 * the border of rhs keeps its content), else GetComponent.  Asynchronous. */
int mf_vsheet_rhs(int sx, int sy, int sz, const float* curl, float* rhs, int c, int shifted, void* stream);

/* vortexplugins.cpp:292-293: solution *= scale, then plane c of vel[3][n] = solution.  Asynchronous. */
int mf_vsheet_set_component(int sx, int sy, int sz, float* vel, float* solution, float scale, int c, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_VSHEET_H */
