/*
 * manta_hip_fields.h -- C ABI extension of `libmanta_hip.so`: three small families of pure grid code of the reference:
 *   fire             source/plugin/fire.cpp (processBurn :22-75, updateFlame :78-90)
 *   wave equation    source/plugin/waves.cpp (calcSecDeriv2d :32-41, totalSum :46-53, normalizeSumTo :56-60, the set-up of cgSolveWE
 *                    :107-126; the solve itself is mf_cg_solve of include/manta_hip.h)
 *   uv grids         source/grid.cpp:573-627 (resetUvGrid, updateUvWeight's two device writes, getUvWeight) and
 *                    extrapolateSimpleFlags, source/plugin/waveletturbulence.cpp:239-307
 * and one host entry, the set-up helper initVortexVelocity (source/plugin/initplugins.cpp:478-503).
 *
 * It lives under include/open/ because the sets of headers include/manta_hip_*.h and include/ext/manta_hip_*.h are both frozen by
 * tests; the rules are those of the other extension headers: include/manta_hip.h and MF_ABI_VERSION stay as they are, a library either
 * implements the whole extension, reporting MF_FIELDS_ABI_VERSION through mf_fields_abi_version(), or none of it.  Conventions (error
 * plumbing, borrowed device pointers, SoA Vec3 grids, idx = i + sx*(j + sy*k), streams) are those of include/manta_hip.h.  The entries do
 * not know the z-slab window (mf_set_slab_window): grids are whole domains.  "Interior" is KERNEL(bnd = 1): 1 <= i < sx-1, 1 <= j < sy-1
 * and, where sz > 1, 1 <= k < sz-1.  Every entry is asynchronous except the two read-backs named below; scratch arrays are the caller's.
 * DESIGN.md section 15 has the fp32 / fp64 map.
 */
#ifndef MANTA_HIP_FIELDS_H
#define MANTA_HIP_FIELDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_fields_process_burn, mf_fields_update_flame, mf_fields_sec_deriv_2d, mf_fields_total_sum, mf_fields_normalize_sum,
 *      mf_fields_wave_system, mf_fields_reset_uv, mf_fields_set_uv_weight, mf_fields_get_uv_weight, mf_fields_extrapolate_mark,
 *      mf_fields_extrapolate_pass, mf_fields_vortex_velocity */
#define MF_FIELDS_ABI_VERSION 1
int mf_fields_abi_version(void);

/* KnProcessBurn on the interior, one kernel; red / green / blue / heat may each be NULL.  fp32 except `(1.0 - origFuel) * 0.5f`, a
 * double expression rounded once.  flame = pow(react, 0.5f) is sqrtf with powf's special cases (-0 -> +0, -inf -> +inf).  The
 * reference's clamp(density, 0, 1) discards its result, so density is not clamped.  Border cells of every grid keep their values. */
int mf_fields_process_burn(int sx, int sy, int sz, float* fuel, float* density, float* react, float* red, float* green, float* blue,
                           float* heat, float burningRate, float flameSmoke, float ignitionTemp, float maxTemp, float dt, float colorX,
                           float colorY, float colorZ, void* stream);

/* KnUpdateFlame on the interior: flame = react > 0 ? pow(react, 0.5f) : 0 */
int mf_fields_update_flame(int sx, int sy, int sz, const float* react, float* flame, void* stream);

/* knCalcSecDeriv2d on the interior (of every plane of a 3-D grid): ret = -4. v + v(i-1) + v(i+1) + v(j-1) + v(j+1), left to right in
 * double, rounded once.  ret must not alias v. */
int mf_fields_sec_deriv_2d(int sx, int sy, int sz, const float* v, float* ret, void* stream);

/* totalSum: the fp64 sum of the interior cells (fixed order of additions, the same on every run), rounded to fp32 into *sum_host.
 * Synchronises the stream: one scalar read-back. */
int mf_fields_total_sum(int sx, int sy, int sz, const float* h, float* sum_host, void* stream);

/* normalizeSumTo: the same sum, factor = float(double(target) / sum) formed on the device, then h *= factor in EVERY cell.  No
 * read-back, no synchronisation. */
int mf_fields_normalize_sum(int sx, int sy, int sz, float* h, float target, void* stream);

/* the set-up of cgSolveWE after MakeLaplaceMatrix, one kernel.  Every cell: Ai, Aj, Ak *= s (fp32), A0 = float(A0 * s) + 1 (two
 * roundings).  Interior: rhs = 2. ut - utm1 in double, rounded once; with crankNic != 0, rhs += s * (-4. ut + 1. ut(i-1) + 1. ut(i+1) +
 * 1. ut(j-1) + 1. ut(j+1)) in double, one more rounding (the 2-D stencil on a 3-D grid as well).  Border: rhs = 0. */
int mf_fields_wave_system(int sx, int sy, int sz, float* A0, float* Ai, float* Aj, float* Ak, float* rhs, const float* ut,
                          const float* utm1, float s, int crankNic, void* stream);

/* knResetUvGrid: uv(i, j, k) = (float(i), float(j), float(k)) + offset in every cell */
int mf_fields_reset_uv(int sx, int sy, int sz, float* uv, float offX, float offY, float offZ, void* stream);

/* uv[0] = (w, 0, 0): the weight updateUvWeight stores in cell 0 of a Vec3 grid of n cells */
int mf_fields_set_uv_weight(int64_t n, float* uv, float w, void* stream);

/* getUvWeight: *w_host = uv[0].x.  Synchronises the stream: one 4-byte read-back. */
int mf_fields_get_uv_weight(const float* uv, float* w_host, void* stream);

/* extrapolateSimpleFlags, the mark pass: tmp = (flags & flagFrom) ? 1 : 0 in every cell */
int mf_fields_extrapolate_mark(int64_t n, const int32_t* flags, int32_t* tmp, int flagFrom, void* stream);

/* extrapolateSimpleFlags, pass d >= 1, on the interior: a cell with tmp == 0 and flags & flagTo sums val of its neighbours with
 * tmp == d in the order +x, -x, +y, -y (, +z, -z where sz > 1); if there are nbs > 0 of them, tmp = d + 1 and val = sum / nbs.
 * ncomp 1 or 3 planes of float (fp32 sum, fp32 division by float(nbs)), or, with isInt != 0, one plane of int32 (int sum, truncating
 * division).  One plain launch, in place: within the pass only cells with tmp == d are read and only cells that become d + 1 are
 * written. */
int mf_fields_extrapolate_pass(int sx, int sy, int sz, const int32_t* flags, int32_t* tmp, void* val, int ncomp, int isInt, int d,
                               int flagTo, void* stream);

/* kninitVortexVelocity on HOST arrays (set-up code; touches no device): in every cell with phiObs >= -1 the x and y planes of vel
 * (3 planes of n floats) are set from i, j alone with the C library's sqrtf / atan2f / sinf / cosf in fp32 */
int mf_fields_vortex_velocity(int sx, int sy, int sz, const float* phiObs_host, float* vel_host, float centerX, float centerY,
                              float radius);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_FIELDS_H */
