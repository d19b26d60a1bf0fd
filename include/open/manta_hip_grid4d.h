/*
 * manta_hip_grid4d.h -- C ABI extension of `libmanta_hip.so`: the 4-D grids of the reference and the arithmetic of its particle data
 * (ParticleDataImpl<T>, source/particle.cpp:434-673; declared at the end),
 *   Grid4d<T>        source/grid4d.{h,cpp} (the broadcast and int forms of the element-wise operators, the reductions, setBound,
 *                    setBoundNeumann, getComp4d / setComp4d, grid4dMaxDiff*, setRegion4d*, getSliceFrom4d*, interpolateGrid4d*)
 *   interpol4d       source/util/vector4d.h:393-442
 * for T = Real, int, Vec3, Vec4.  The flat float operators (add, sub, mult, clamp, ... of Real grids and of whole Vec grids) are the
 * mf_grid_* / mf_fill_* entries of include/manta_hip.h with n = ncomp * sx*sy*sz*st and are not repeated here.
 *
 * The rules are those of the other extension headers: include/manta_hip.h and MF_ABI_VERSION stay as they are, a library either
 * implements the whole extension, reporting MF_GRID4D_ABI_VERSION through mf_grid4d_abi_version(), or none of it.  Conventions (error
 * plumbing, borrowed device pointers, streams) are those of include/manta_hip.h.  A 4-D grid of ncomp components is ncomp planes of
 * n = sx*sy*sz*st words (structure of arrays), idx = i + sx*(j + sy*(k + sz*t)); n stays below 2^31.  The entries do not know the
 * z-slab window: grids are whole domains.  Every entry is asynchronous except the reductions, which read scalars back and say so.
 * DESIGN.md section 19 has the fp32 / fp64 map.
 *
 * Preconditions (the caller's; the entries check what they can see):
 *   - every axis of an interpolation source has at least 2 cells (interpol4d indexes size - 2): checked, refused;
 *   - mf_grid4d_set_bound_neumann needs every axis >= 2 * w + 3 cells: below that a cell's source is itself a boundary cell and the
 *     reference's in-place kernel depends on the order of its threads: checked, refused;
 *   - the inputs of the min / max reductions hold no NaN (the reference's `<` / `>` folds and fminf / fmaxf differ there): unchecked.
 */
#ifndef MANTA_HIP_GRID4D_H
#define MANTA_HIP_GRID4D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_grid4d_vec_const, mf_grid4d_vec_scaled_add, mf_grid4d_int_const, mf_grid4d_int_binary, mf_grid4d_int_clamp,
 *      mf_grid4d_int_min_max, mf_grid4d_norm_min_max, mf_grid4d_max_diff, mf_grid4d_set_bound, mf_grid4d_set_bound_neumann,
 *      mf_grid4d_get_comp, mf_grid4d_set_comp, mf_grid4d_set_region, mf_grid4d_get_slice, mf_grid4d_interpolate,
 *      mf_grid4d_pdata_set_flag, mf_grid4d_pdata_clamp_side, mf_grid4d_pdata_sum, mf_grid4d_pdata_set_noise,
 *      mf_grid4d_check_symmetry, mf_grid4d_init_grid_with_pos */
#define MF_GRID4D_ABI_VERSION 1
int mf_grid4d_abi_version(void);

/* kn4dSetConstReal / kn4dAddConstReal / kn4dMultConst for T = Vec3 (ncomp 3) or Vec4 (ncomp 4): op 0 me = v, 1 me += v, 2 me *= v,
 * component c of every cell with v[c] = (vx, vy, vz, vt)[c]; fp32 */
int mf_grid4d_vec_const(int op, int ncomp, int64_t n, float* me, float vx, float vy, float vz, float vt, void* stream);

/* Grid4dScaledAdd<T, T> for T = Vec3 / Vec4: me += factor * other per component, the product rounded to fp32 before the sum */
int mf_grid4d_vec_scaled_add(int ncomp, int64_t n, float* me, const float* other, float fx, float fy, float fz, float ft, void* stream);

/* the int forms: op 1 me += v, 2 me *= v (op 0, me = v, is mf_fill_i32); two's-complement wrap-around */
int mf_grid4d_int_const(int op, int64_t n, int32_t* me, int32_t v, void* stream);
/* op 0 me += other, 1 me -= other, 2 me *= other, 3 me += factor * other, 4 me = other ? me / other : me (safeDivide<int>; the one
 * quotient C leaves undefined, INT_MIN / -1, wraps to INT_MIN) */
int mf_grid4d_int_binary(int op, int64_t n, int32_t* me, const int32_t* other, int32_t factor, void* stream);
/* kn4dClamp<int>: me = me < lo ? lo : (me > hi ? hi : me) */
int mf_grid4d_int_clamp(int64_t n, int32_t* me, int32_t lo, int32_t hi, void* stream);
/* kn4dMinInt / kn4dMaxInt in one pass.  Synchronises the stream: two scalars are read back. */
int mf_grid4d_int_min_max(int64_t n, const int32_t* a, int32_t* min_host, int32_t* max_host, void* stream);

/* kn4dMinVec / kn4dMaxVec for ncomp 3 or 4 (and CompPdata_MinVec3 / MaxVec3 of particle.cpp): the smallest and the largest normSquare,
 * x*x + y*y + z*z (+ t*t) in fp32 from left to right (no square root: the caller takes it), over n items of component planes `stride`
 * words apart (a grid: stride == n; particle data: the capacity).  Synchronises the stream: two scalars are read back. */
int mf_grid4d_norm_min_max(int ncomp, int64_t n, int64_t stride, const float* a, float* min_host, float* max_host, void* stream);

/* grid4dMaxDiff (ncomp 1, isInt 0: |a - b| formed in fp32, widened), grid4dMaxDiffInt (ncomp 1, isInt 1: |double(a) - b|),
 * grid4dMaxDiffVec3 / Vec4 (ncomp 3 / 4: the per-cell sum over c of |double(a_c) - double(b_c)|, c ascending); the maximum over the
 * cells in fp64, started from 0.  A maximum does not depend on the order: exact.  Synchronises the stream: one scalar read back. */
int mf_grid4d_max_diff(int ncomp, int isInt, int64_t n, const void* a, const void* b, double* result_host, void* stream);

/* knSetBnd4d: every cell with i <= w, i >= sx-1-w, or the same on j, k, t, takes the value: component c gets word c of the four
 * 32-bit words v0..v3 (float bits or ints: the words are stored as they are) */
int mf_grid4d_set_bound(int sx, int sy, int sz, int st, void* grid, int ncomp, int32_t v0, int32_t v1, int32_t v2, int32_t v3, int w,
                        void* stream);

/* knSetBnd4dNeumann: such a cell takes the words of the cell whose every out-of-range coordinate is moved to w+1 or size-w-2.
 * In place in one launch: with every axis >= 2w+3 no source cell is a boundary cell.  w >= 0. */
int mf_grid4d_set_bound_neumann(int sx, int sy, int sz, int st, void* grid, int ncomp, int w, void* stream);

/* knGetComp4d: dst = plane c of a Vec4 grid; knSetComp4d: plane c of dst = src.  0 <= c < 4 */
int mf_grid4d_get_comp(int64_t n, const float* src4, float* dst, int c, void* stream);
int mf_grid4d_set_comp(int64_t n, const float* src, float* dst4, int c, void* stream);

/* knSetRegion4d: cells whose float coordinates p = (i, j, k, t) have start[c] <= p[c] <= end[c] for every c (the negation of
 * `p[c] < start[c] || p[c] > end[c]`) take the value; ncomp 1 (v0) or 4 */
int mf_grid4d_set_region(int sx, int sy, int sz, int st, float* grid, int ncomp, float s0, float s1, float s2, float s3, float e0,
                         float e1, float e2, float e3, float v0, float v1, float v2, float v3, void* stream);

/* getSliceFrom4d (ncomp 1: dst one plane) / getSliceFrom4dVec (ncomp 4: dst three planes of dn = dx*dy*dz words, dstt one plane or
 * NULL): dst(i, j, k) = src(i, j, k, srct) where (i, j, k) lies in both grids; nothing happens when srct is outside [0, st) */
int mf_grid4d_get_slice(int sx, int sy, int sz, int st, const float* src, int ncomp, int srct, int dx, int dy, int dz, float* dst,
                        float* dstt, void* stream);

/* knInterpol4d for Real (ncomp 1) and Vec4 (ncomp 4; the vector expression is the scalar one per component):
 * pos = (i, j, k, t) * fac + off in fp32 (a product and a sum, two roundings), target = interpol4d(source, pos): p = pos - 0.5f, the
 * cell (int)p, weights s1 = p - cell, s0 = float(1. - s1); p < 0 gives cell 0 with weights (1, 0), cell >= size-1 gives cell size-2
 * with weights (0, 1) -- the lower rule looks at the position, the upper one at the index; the 16 corners are combined with the
 * reference's bracketing, y inside x inside z inside t, in fp32 without contraction.  fac and off are gridFactor4d's, formed by the
 * caller.  target must not alias source. */
int mf_grid4d_interpolate(int tx, int ty, int tz, int tt, float* target, int sx, int sy, int sz, int st, const float* source, int ncomp,
                          float f0, float f1, float f2, float f3, float o0, float o1, float o2, float o3, void* stream);

/* ---- particle data (source/particle.cpp:434-673): channels are component planes `stride` words apart, the live slots are [0, n);
 * n may be 0 (nothing is launched); slots at and past n are never touched.  The flat float operators of a channel are the mf_grid_*
 * entries of include/manta_hip.h on each plane; the int forms are mf_grid4d_int_* above (one plane). ---- */

/* knPdataSetScalarIntFlag: slots with t[idx] & itype take the value, component c the 32-bit word w_c (float bits or an int) */
int mf_grid4d_pdata_set_flag(int64_t n, int64_t stride, int ncomp, void* me, int32_t w0, int32_t w1, int32_t w2, const int32_t* t,
                             int itype, void* stream);

/* knPdataClampMin (side 0: me = std::max(v, me), i.e. v < me ? me : v) and knPdataClampMax (side 1: me = std::min(v, me), i.e.
 * me < v ? me : v), every component against the same v (knPdataClampMinVec3 / MaxVec3); v is a float's word, or an int where isInt */
int mf_grid4d_pdata_clamp_side(int side, int isInt, int64_t n, int64_t stride, int ncomp, void* me, int32_t v, void* stream);

/* KnPtsSum (what 0; t may be NULL: every slot, else the slots with t[idx] & itype), KnPtsSumSquare (1), KnPtsSumMagnitude (2).
 * The reference adds Reals in slot order on one thread, which no parallel sum reproduces bit for bit.  Contract: the terms are the
 * reference's fp32 terms (normSquare in fp32 from left to right; norm() of a Vec3 is 0 where l <= 1e-12f, 1 where |l - 1.| < 1e-12,
 * else sqrtf(l); int terms are converted as Real(v * v) / Real(abs(v))), accumulated in fp64 in a fixed order (per-thread strided
 * partial sums, a fixed tree per block, one finishing block) and rounded once to fp32: the same bits on every run, equal to the
 * reference wherever every partial sum of the reference is exact, and within gamma(n-1) * sum|term| + 2^-24 |S| of it otherwise.
 * An int channel's sum (what 0, isInt) is exact, wrapped to 32 bits like the reference's.  result_host: ncomp words for what 0 (floats,
 * or one int), one float otherwise.  Synchronises the stream: the scalars are read back. */
int mf_grid4d_pdata_sum(int what, int isInt, int ncomp, int64_t n, int64_t stride, const void* a, const int32_t* t, int itype,
                        void* result_host, void* stream);

/* knSetPdataNoise / knSetPdataNoiseVec (plugin/initplugins.cpp:53-64), one thread per slot: kind 0 Real pd = evaluate(pos) * scale,
 * kind 1 int pd = int(evaluate(pos) * scale) (truncation), kind 2 Vec3 pd = evaluateVec(pos) * scale, with WaveletNoiseField::evaluate /
 * evaluateVec as mf_add_noise and mf_apply_noise_vec3 evaluate them (tile 0 of the 3 x 128^3 noise tile, the parameter block of
 * mf_density_inflow: host floats).  pos: 3 planes pstride apart; pd: planes stride apart.  fp32 throughout. */
int mf_grid4d_pdata_set_noise(int kind, int64_t n, int64_t stride, void* pd, int64_t pstride, const float* pos, const float* tile,
                              const float* params, float scale, void* stream);

/* ---- three helpers of the reference's test harness on 3-D / 2-D grids (idx = i + sx*(j + sy*k)) ---- */

/* checkSymmetry (mac 0: a one plane) and checkSymmetryVec3 (mac 1: a three planes; err is first set to 0, then the sweeps of the
 * normal component `axis` -- mirrored about size + 1 with its sign flipped, the centre line compared with and set to 0 -- and of the
 * two other components add up; bit q of disable drops sweep q).  err (nullable) = |a(idx) - a(mirror)| with the reference's
 * promotions (scalar and tangential: fp32 difference; normal: the double sum; `err +=` rounds double(err) + e once).  With
 * symmetrize the cells below the middle take their mirror's value; the reference's serial loop lets cells at and above the middle
 * see those new values, which is restated as two passes per sweep.  bound > 0 skips pairs with a cell
 * within `bound` of the sides.  axis 0..2. */
int mf_grid4d_check_symmetry(int sx, int sy, int sz, float* a, int mac, float* err, int symmetrize, int axis, int bound, int disable,
                             void* stream);

/* testInitGridWithPos (plugin/flip.cpp:191-193): grid(i, j, k) = norm(Vec3(i, j, k)), fp32 */
int mf_grid4d_init_grid_with_pos(int sx, int sy, int sz, float* grid, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_GRID4D_H */
