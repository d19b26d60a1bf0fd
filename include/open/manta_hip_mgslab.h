/*
 * manta_hip_mgslab.h -- C ABI extension of `libmanta_hip.so`: the V-cycle of the multigrid preconditioner (mantaflow's GridMg,
 * source/multigrid.{h,cpp}) with level 0 cut into ranges of z-planes, for the z-slab pressure solve (mantaflow_amd/slab.py).
 *
 * It sits beside include/manta_hip_multigrid.h, takes the handles of mf_mg_create and leaves that header, its entries and its
 * revision as they are: a library either implements this whole extension, reporting MF_MGSLAB_ABI_VERSION through
 * mf_mgslab_abi_version(), or none of it.  Conventions (error plumbing, borrowed device pointers, idx = i + sx*(j + sy*k),
 * streams) are those of include/manta_hip.h.
 *
 * The form.  Every rank holds a whole-domain hierarchy with the same matrix (mf_mg_set_a on the gathered system).  A rank
 * that owns the fine planes [z0, z1) runs the level-0 passes of doVCycle (multigrid.cpp:417-504) on those planes only, on
 * the handle's whole-domain level-0 arrays; between the passes the caller moves single planes of x and r between the ranks
 * (mf_mgslab_get_planes / _put_planes are the device-side staging).  Restriction fills the coarse planes a rank owns, the
 * caller gathers b of level 1, and the levels 1 .. L-1 run replicated on every rank by mf_mgslab_coarse: the code of
 * mf_mg_vcycle.  No pass has a dependency between the vertices it writes, and a ranged pass is the whole-grid pass on a
 * sub-range of its work items (one definition, mg3d_cells.h), so the planes a rank owns come out with the bits of
 * mf_mg_vcycle on the undivided grid, for any number of ranks and any cut.
 *
 * Every entry refuses, by name and before it touches memory: a destroyed or foreign handle (a 2-D handle of mf_mg2d_create
 * is one), a handle whose matrix has not been set, and a plane range outside 0 <= z0 <= z1 <= sz of the level.  An empty
 * range (z0 == z1) is a no-op.  A plane range is always [z0, z1) in planes of the level it names.
 */
#ifndef MANTA_HIP_MGSLAB_H
#define MANTA_HIP_MGSLAB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  set_accuracy / set_rhs / smooth / residual / restrict / coarse / interp_add / get_planes / put_planes */
#define MF_MGSLAB_ABI_VERSION 1
int mf_mgslab_abi_version(void);

/* mCoarsestLevelAccuracy = accuracy * 1e-4, what InitPreconditionMultigrid (conjugategrad.cpp:100-106) sets inside
 * mf_mg_cg_solve: the slab PCG does not go through that entry. */
int mf_mgslab_set_accuracy(void* handle, float accuracy);

/* knSetRhs + knSet(x_0, 0), multigrid.cpp:417-424, 458, on the fine planes [z0, z1): b from `rhs`, which holds those planes
 * only ((z1 - z0) * sx * sy floats, plane z0 first).  x_0 is zeroed on [z0, z1) and on the planes z0 - 1 and z1 where they
 * exist (the ghost planes the first smoothing colour reads). */
int mf_mgslab_set_rhs(void* handle, int z0, int z1, const float* rhs, void* stream);

/* knSmoothColor, multigrid.cpp:668-711: colour `colour` (0 or 1, the parity of x + y + z) of level 0 on the planes [z0, z1).
 * Reads x on z0 - 1 and z1. */
int mf_mgslab_smooth(void* handle, int colour, int z0, int z1, void* stream);

/* knCalcResidual, multigrid.cpp:739-771: r of level 0 on the planes [z0, z1).  Reads x on z0 - 1 and z1. */
int mf_mgslab_residual(void* handle, int z0, int z1, void* stream);

/* knRestrict, multigrid.cpp:904-927: b of level 1 on the COARSE planes [k0, k1) from r of level 0 (coarse plane K reads the
 * fine planes 2K - 1 .. 2K + 1 that exist). */
int mf_mgslab_restrict(void* handle, int k0, int k1, void* stream);

/* Levels 1 .. L-1 of doVCycle, down and up again (multigrid.cpp:460-494), whole on this device, as mf_mg_vcycle queues them:
 * x of level 1 is zeroed first (knSet, :472), b of level 1 must be complete.  Refuses a hierarchy whose level 0 runs inside
 * the single-workgroup tail (mf_mg_info slot [5] == 0, one-level hierarchies among them): such a hierarchy is not cut. */
int mf_mgslab_coarse(void* handle, void* stream);

/* knInterpolate + knAddAssign, multigrid.cpp:484-486, 934-954: x of level 0 on the planes [z0, z1) += the interpolated x of
 * level 1 (fine plane Z reads the coarse planes Z / 2 .. (Z + 1) / 2). */
int mf_mgslab_interp_add(void* handle, int z0, int z1, void* stream);

/* Device-to-device copies of the planes [z0, z1) of one vector of level `level` out of / into a caller tensor of
 * (z1 - z0) * sx * sy floats of that level: what = 2 x, 3 b (the numbers of mf_mg_read_level), 4 r. */
int mf_mgslab_get_planes(void* handle, int level, int what, int z0, int z1, float* dst, void* stream);
int mf_mgslab_put_planes(void* handle, int level, int what, int z0, int z1, const float* src, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_MGSLAB_H */
