/*
 * manta_hip_guiding.h -- C ABI extension of `libmanta_hip.so`: the pieces of source/plugin/fluidguiding.cpp (Inglis et al.,
 * "Primal-Dual Optimization for Fluids") around its inner solvePressure: the 1-D Gaussian weights (:31-45), the separable blur of a
 * MAC grid with its obstacle restore (:49-136), precomputeInvA (:254-263), and the element-wise chains of one primal-dual iteration
 * (:229-239, :266-271, :323-344) fused into three kernels, the last of which also yields the two maxima of the stop test.
 *
 * It sits beside include/manta_hip.h and leaves that header (and MF_ABI_VERSION) as it is: a library either implements the whole
 * extension, reporting MF_GUIDING_ABI_VERSION through mf_guiding_abi_version(), or none of it.  Conventions (error plumbing, borrowed
 * device pointers, SoA Vec3 grids [3][n], idx = i + sx*(j + sy*k), streams) are those of include/manta_hip.h.  The entries do not
 * know the z-slab window (mf_set_slab_window): grids are whole domains.  Every entry but mf_guiding_weights (host only) and
 * mf_guiding_post (one read-back of two floats) is asynchronous on the stream.
 *
 * All arithmetic is fp32, one rounding per operation of the reference's chain of grid methods, no contraction; scalars arrive
 * already rounded to fp32 where the reference passes them as Real or Vec3.
 */
#ifndef MANTA_HIP_GUIDING_H
#define MANTA_HIP_GUIDING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_guiding_weights, mf_guiding_blur, mf_guiding_inv_a, mf_guiding_pre, mf_guiding_mid, mf_guiding_post */
#define MF_GUIDING_ABI_VERSION 1
int mf_guiding_abi_version(void);

/* get1DGaussianBlurKernel(n, n) with n = 2*radius+1 (:31-45), host code with the host C library's expf: w_host[0 .. 2*radius].
 * The reference keeps the kernel in a sparse fp32 matrix that drops every value with |v| <= 1e-6 on insertion (util/rcmatrix.h:
 * 186-187); such a weight is 0 here.  0 <= radius <= 1024. */
int mf_guiding_weights(int radius, float* w_host);

/* applySeparableKernel2D / 3D (:87-130), `times` in a row, in place on grid [3][n].
 *   w_dev   : the 2*radius+1 weights, on the device
 *   s1, s2  : scratch [3][n], any content on entry; s2 may be NULL when sz == 1 (no z pass)
 * Per 1-D pass, cell and component: acc = 0; for m = 0 .. kn-1: acc += in[tap m] * w[kn-1-m], taps outside the grid skipped.  After
 * the last pass of each blur a cell that is an obstacle, or whose lower x / y / (3-D) z neighbour is one, keeps its value from
 * before that blur. */
int mf_guiding_blur(int sx, int sy, int sz, const int32_t* flags, float* grid, float* s1, float* s2, const float* w_dev, int radius,
                    int times, void* stream);

/* precomputeInvA (:254-263), one float per cell (the reference's three components are equal):
 * val = 2*w*w + sigma; if (val < 0.01) val = 0.01; invA = 1.0 / val */
int mf_guiding_inv_a(int64_t n, const float* weight, float sigma, float* invA, void* stream);

/* The x update up to the blurs (:324-326, :267-268, :230-232), per component:
 *   xv = ((x * inv_sigma + y) * sigma) + Q        vn = xv * invA
 * x, y, Q, xv, vn: [3][n]; invA: [n].  x is left as it is (it is the x0 of :323). */
int mf_guiding_pre(int64_t n, const float* x, const float* y, const float* Q, const float* invA, float* xv, float* vn, float inv_sigma,
                   float sigma, void* stream);

/* The x update after the blurs and the z update (:235-238, :270, :327-331), per component, vn being the twice-blurred grid:
 *   x  = ((((xv * invA) - ((vn * 2) * invA)) + velC) * (-sigma) + sigma * y) + x
 *   zn = z + (-tau) * x
 * zn is the new slack grid, z becomes the z0 of :330 (the caller swaps). */
int mf_guiding_mid(int64_t n, float* x, const float* y, const float* xv, const float* vn, const float* invA, const float* velC,
                   const float* z, float* zn, float sigma, float tau, void* stream);

/* The y update and the maxima of the stop test (:338-344) after the solve:
 *   y = ((z - z0) * theta) + z
 *   out_host[0] = sqrt(max normSquare(z - z0))   (getRNorm; the difference rounded per component)
 *   out_host[1] = sqrt(max normSquare(z))        (Grid<Vec3>::getMaxAbs, grid.cpp:222-226, :367-369)
 * Synchronises the stream: the one read-back of a primal-dual iteration. */
int mf_guiding_post(int64_t n, const float* z, const float* z0, float* y, float theta, float* out_host, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_GUIDING_H */
