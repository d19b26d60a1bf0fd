/*
 * manta_hip_mg2d.h -- C ABI extension of `libmanta_hip.so`: the multigrid preconditioner of the pressure PCG on 2-D grids
 * (mantaflow's GridMg in its 2-D mode, source/multigrid.{h,cpp}: mIs3D == false, multigrid.cpp:231-236 -- a 5-point stencil
 * in 3 stored entries on level 0, a 9-point stencil in 5 stored entries above it, two colours of the smoother on level 0 and
 * four above, :723-726).
 *
 * It sits beside include/manta_hip_multigrid.h (the 3-D hierarchy), mirrors its entries one for one and leaves that header,
 * its entries and mf_mg_create's refusal of sz <= 1 as they are: a library either implements this whole extension, reporting
 * MF_MG2D_ABI_VERSION through mf_mg2d_abi_version(), or none of it.  Conventions (error plumbing, borrowed device pointers,
 * idx = i + sx*j, streams) are those of include/manta_hip.h.  Every entry cites the reference lines it reproduces, bit for bit:
 * fp32 in the reference's operation order, the coarsest-level CG in fp64 with its sums in vertex order.
 *
 * What runs: 2-D grids (sx x sy x 1) on one device, any matrix solvePressure can assemble (fractions, ghost fluid, zero
 * pressure fixing).  What does not: z-slab windows (mf_set_slab_window is not consulted) and the CPU oracle backend, which
 * lacks the extension.  The Python layer reaches these entries only after mantaflow_amd.multigrid2d.setMultigrid2D().
 *
 * A hierarchy is a handle owned by the caller; the library keeps no global multigrid state.  A handle belongs to the device
 * that was current when it was created.  A destroyed handle, or a pointer this extension did not hand out (a 3-D handle of
 * mf_mg_create among them), is refused by name without its memory being read.
 */
#ifndef MANTA_HIP_MG2D_H
#define MANTA_HIP_MG2D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  create / destroy / set_a / is_a_set / vcycle / cg_solve / info / read_level */
#define MF_MG2D_ABI_VERSION 1
int mf_mg2d_abi_version(void);

/* GridMg::GridMg with gridSize.z == 1, multigrid.cpp:220-319: the level pyramid (sizes ((sx + 2) / 2, (sy + 2) / 2, 1); no
 * further level once both axes are <= 5 or the level has <= 1000 vertices, :256-276) with device buffers for A, x, b, r and
 * the vertex types of every level, and the sorted coarsening paths of level 1 (:286-318 with mDim = 2: U in 3 x 3, five
 * p7stencil entries, sc = s - 13 in 0..4).  *handle_out receives the handle. */
int mf_mg2d_create(int sx, int sy, void** handle_out);
int mf_mg2d_destroy(void* handle);

/* GridMg::setA, multigrid.cpp:386-414: copies the 3-entry level-0 stencil (knCopyA, :351-358; the caller's grids are not
 * modified), marks the vertex types (knActivateVertices / analyzeStencil with A[3] = A[6] = 0, :321-384; trivial equations
 * 1 * x = b are scaled by 1e-6), then per coarse level selects the coarse vertices (genCoarseGrid, :520-578 -- the serial
 * greedy selection runs on the host, in the reference's heap order, on the downloaded type array) and builds the Galerkin
 * operator on the device (knGenCoarseGridOperator, :580-657: level 1 summed in the order of the sorted paths, the levels
 * above over the 9-point neighbourhood).  Synchronises the stream. */
int mf_mg2d_set_a(void* handle, const float* A0, const float* Ai, const float* Aj, void* stream);
/* GridMg::isASet, multigrid.h:47: returns 1 / 0 (not an error code); -1 for a bad handle */
int mf_mg2d_is_a_set(void* handle);

/* ApplyPreconditionMultigrid, conjugategrad.cpp:162-167: setRhs(rhs) + doVCycle(dst) with a zero initial guess and (1, 1)
 * smoothing (multigrid.cpp:417-504, :668-960).  The coarsest-level CG (solveCG, :796-902) runs to the relative accuracy set
 * by the last mf_mg2d_cg_solve (1e-8 before any).  The residual norm doVCycle returns is not computed.  dst and rhs: sx*sy
 * floats each; they may not alias. */
int mf_mg2d_vcycle(void* handle, float* dst, const float* rhs, void* stream);

/* GridCg<ApplyMatrix2D>::doInit / iterate with PC_MGP, conjugategrad.cpp:216-300: mf_cg_solve (manta_hip.h) on the grid
 * sx x sy x 1 without an Ak, with the hierarchy in place of Aprecond / pc.  InitPreconditionMultigrid (:100-106): set_a only
 * when the handle has no matrix yet -- a handle that has one keeps it, whatever A0..Aj hold (PcMGStatic) -- and the coarsest
 * accuracy becomes accuracy * 1e-4.  out_host[3] = {iterations, residual norm, sigma}. */
int mf_mg2d_cg_solve(void* handle, int sx, int sy, const int32_t* flags, float* dst, const float* rhs, float* residual,
                     float* search, float* tmp, const float* A0, const float* Ai, const float* Aj, float accuracy,
                     int maxIter, int useL2Norm, float* out_host, void* stream);

/* What tests and timing tools need to see; the slots of mf_mg_info (the debug messages of multigrid.cpp:399-402 are slots 3
 * and 4).  out_host[0] = number of levels L, [1] = number of set_a runs so far, [2] = iterations of the coarsest-level CG in
 * the last V-cycle, [3] = 1 when the last set_a found a row with a non-zero stencil sum (0: the reference warns of a constant
 * mode), [4] = 1 when it found trivial equations, [5] = first level of the fused single-workgroup tail of the V-cycle,
 * [6] / [7] = microseconds the last set_a spent in the host selection / in everything else, then per level l:
 * [8 + 4 l ..] = sx, sy, 1, active vertices.  n_out >= 8 + 4 L (L <= 16).  Synchronises the device. */
int mf_mg2d_info(void* handle, int64_t* out_host, int n_out);

/* Copies one array of level `level` to host memory: what = 0 vertex types (1 byte per vertex: 0 inactive, 1 active, 2 active
 * trivial), 1 the operator (level 0: 3 planes A0, Ai, Aj with the scaled trivial rows; levels > 0: 5 planes, plane s the
 * stored entry s of the symmetric 9-point stencil -- the z = 0 slice of multigrid.cpp:214-218: 0 centre, 1 (+1, 0),
 * 2 (-1, +1), 3 (0, +1), 4 (+1, +1)), 2 x, 3 b.  bytes must be the exact size.  Synchronises the device. */
int mf_mg2d_read_level(void* handle, int level, int what, void* dst_host, int64_t bytes);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_MG2D_H */
