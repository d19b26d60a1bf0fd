/*
 * manta_hip_multigrid.h -- C ABI extension of `libmanta_hip.so`: the multigrid preconditioner of the pressure PCG
 * (mantaflow's GridMg, source/multigrid.{h,cpp}: solvePressure(preconditioner = PcMGDynamic | PcMGStatic)).
 *
 * It sits beside include/manta_hip.h and leaves that header (and MF_ABI_VERSION) as it is: a library either
 * implements the whole extension, reporting MF_MULTIGRID_ABI_VERSION through mf_multigrid_abi_version(), or none
 * of it.  Conventions (error plumbing, borrowed device pointers, idx = i + sx*(j + sy*k), streams) are those of
 * include/manta_hip.h.  Every entry cites the reference lines it reproduces, bit for bit: fp32 in the reference's
 * operation order, the coarsest-level CG in fp64 with its sums in vertex order.
 *
 * What runs: 3-D grids (sz > 1) on one device, any matrix solvePressure can assemble (fractions, ghost fluid, zero
 * pressure fixing).  What does not: 2-D grids (the reference's 5/9-point, 4-colour variant), z-slab windows
 * (mf_set_slab_window is not consulted: grids are whole domains), and the CPU oracle backend, which lacks the extension.
 *
 * A hierarchy is a handle owned by the caller (one per FluidSolver in the Python layer); the library keeps no global
 * multigrid state.  A handle belongs to the device that was current when it was created.
 */
#ifndef MANTA_HIP_MULTIGRID_H
#define MANTA_HIP_MULTIGRID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  create / destroy / set_a / vcycle / cg_solve / info / read_level */
#define MF_MULTIGRID_ABI_VERSION 1
int mf_multigrid_abi_version(void);

/* GridMg::GridMg, multigrid.cpp:220-319: the level pyramid (sizes (s + 2) / 2 per axis; no further level once every axis is <= 5
 * or the level has <= 1000 vertices) with device buffers for A, x, b, r and the vertex types of every level, and the sorted
 * coarsening paths of level 1.  *handle_out receives the handle.  sz must be > 1. */
int mf_mg_create(int sx, int sy, int sz, void** handle_out);
int mf_mg_destroy(void* handle);

/* GridMg::setA, multigrid.cpp:386-414: copies the level-0 stencil (the caller's grids are not modified), marks the vertex
 * types (knActivateVertices; trivial equations 1 * x = b are scaled by 1e-6), then per coarse level selects the coarse
 * vertices (genCoarseGrid, :520-578 -- the serial greedy selection runs on the host, in the reference's heap order, on the
 * downloaded type array) and builds the Galerkin operator on the device (knGenCoarseGridOperator, :580-657, summed in the
 * order of the sorted paths).  Synchronises the stream. */
int mf_mg_set_a(void* handle, const float* A0, const float* Ai, const float* Aj, const float* Ak, void* stream);
/* GridMg::isASet: returns 1 / 0 (not an error code); -1 for a bad handle */
int mf_mg_is_a_set(void* handle);

/* ApplyPreconditionMultigrid, conjugategrad.cpp:162-167: setRhs(rhs) + doVCycle(dst) with a zero initial guess and (1, 1)
 * smoothing (multigrid.cpp:417-504, :668-960).  The coarsest-level CG (solveCG, :796-902) runs to the relative accuracy set
 * by the last mf_mg_cg_solve (1e-8 before any).  The residual norm doVCycle returns is not computed.  dst and rhs: sx*sy*sz
 * floats each; they may not alias. */
int mf_mg_vcycle(void* handle, float* dst, const float* rhs, void* stream);

/* GridCg::doInit / iterate with PC_MGP, conjugategrad.cpp:216-300: mf_cg_solve (manta_hip.h) with the hierarchy in place of
 * Aprecond / pc.  InitPreconditionMultigrid (:100-106): set_a only when the handle has no matrix yet -- a handle that has one
 * keeps it, whatever A0..Ak hold (PcMGStatic) -- and the coarsest accuracy becomes accuracy * 1e-4.
 * out_host[3] = {iterations, residual norm, sigma}. */
int mf_mg_cg_solve(void* handle, int sx, int sy, int sz, const int32_t* flags, float* dst, const float* rhs, float* residual,
                   float* search, float* tmp, const float* A0, const float* Ai, const float* Aj, const float* Ak, float accuracy,
                   int maxIter, int useL2Norm, float* out_host, void* stream);

/* What tests and timing tools need to see.  out_host[0] = number of levels L, [1] = number of set_a runs so far, [2] = iterations
 * of the coarsest-level CG in the last V-cycle, [3] = 1 when the last set_a found a row with a non-zero stencil sum (0: the
 * reference warns of a constant mode), [4] = 1 when it found trivial equations, [5] = first level of the fused single-workgroup
 * tail of the V-cycle, [6] / [7] = microseconds the last set_a spent in the host selection / in everything else, then per
 * level l: [8 + 4 l ..] = sx, sy, sz, active vertices.  n_out >= 8 + 4 L (L <= 16).  Synchronises the device. */
int mf_mg_info(void* handle, int64_t* out_host, int n_out);

/* Copies one array of level `level` to host memory: what = 0 vertex types (1 byte per vertex: 0 inactive, 1 active, 2 active
 * trivial), 1 the operator (level 0: 4 planes A0, Ai, Aj, Ak with the scaled trivial rows; levels > 0: 14 planes, plane s the
 * stencil entry s of multigrid.cpp:214-218), 2 x, 3 b.  bytes must be the exact size.  Synchronises the device. */
int mf_mg_read_level(void* handle, int level, int what, void* dst_host, int64_t bytes);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_MULTIGRID_H */
