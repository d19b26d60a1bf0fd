/*
 * manta_hip_datagen.h -- C ABI extension of `libmanta_hip.so`: the plugins a smoke scene uses to turn a fine simulation into training
 * data and pictures:
 *   Gaussian blurs     source/plugin/initplugins.cpp:510-655 (GaussianKernelCreator, knBlurGrid, KnBlurMACGridGauss)
 *   centre of mass     source/plugin/initplugins.cpp:337-348 (calcCenterOfMass)
 *   ppm projection     source/util/simpleimage.cpp:20-67, 206-281 and simpleimage.h:46-50, 110-117 (projectImg, writePpm's bytes)
 *   Laplacian          LaplaceOp, source/commonkernels.h:75-80
 *   curvature          CurvatureOp, source/commonkernels.h:83-101
 *
 * It lives under include/open/ with the other open extensions and follows their rules: include/manta_hip.h and MF_ABI_VERSION stay as
 * they are, a library either implements the whole extension, reporting MF_DATAGEN_ABI_VERSION through mf_datagen_abi_version(), or
 * none of it.  Conventions (error plumbing, borrowed device pointers, SoA Vec3 grids, idx = i + sx*(j + sy*k), a stream as the last
 * argument) are those of include/open/manta_hip_fields.h.  The entries do not know the z-slab window: grids are whole domains.
 * "Interior" is KERNEL(bnd = 1): 1 <= i < sx-1, 1 <= j < sy-1 and, where sz > 1, 1 <= k < sz-1.  Every entry is asynchronous except the
 * read-back named below; scratch arrays are the caller's.  DESIGN.md section 23 has the fp32 / fp64 map.
 */
#ifndef MANTA_HIP_DATAGEN_H
#define MANTA_HIP_DATAGEN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* revision of this extension; a loader binds the entries below only when the library reports the revision it was built against
 *   1  mf_datagen_weights, mf_datagen_blur, mf_datagen_center_of_mass, mf_datagen_project, mf_datagen_laplacian,
 *      mf_datagen_curvature */
#define MF_DATAGEN_ABI_VERSION 1
int mf_datagen_abi_version(void);

/* the longest blur kernel an entry takes: the weights travel as a kernel argument (sigma up to about 42) */
#define MF_DATAGEN_MAX_TAPS 255

/* GaussianKernelCreator::setGaussianSigma on the HOST (no device is touched): *mdim_host = mDim = (int)(2.0 * 3.0 * sigma + 1.0f), at
 * least 3, made odd; w_host[c +- i] = float(m * exp(-(1.0*i*i) / (2.0 * s2))) with c = mDim / 2, s2 = sigma * sigma in fp32,
 * m = float(1.0 / (sqrt(2.0 * M_PI) * sigma)) and the C library's exp.  Not normalised.  w_host has room for cap floats; sigma must be
 * finite and positive and mDim at most min(cap, MF_DATAGEN_MAX_TAPS). */
int mf_datagen_weights(float sigma, int cap, float* w_host, int* mdim_host);

/* blurRealGrid (ncomp 1) / blurMacGrid (ncomp 3, every component at the cell's own index): separable passes x, y and, where sz > 1, z
 * with the weights above.  One pass: acc = 0; acc += w[d] * src[clamp(pos - (d - mDim/2) e_dir)] for d = 0 .. mDim-1, product and sum
 * rounded separately in fp32, the tap index clamped to [0, size-1].  src -> tmpA -> dst (2-D), src -> tmpA -> tmpB -> dst (3-D); tmpA,
 * tmpB (NULL allowed in 2-D): ncomp * n floats each, distinct from src and dst.  dst may be src.  *mdim_host = mDim.  Asynchronous. */
int mf_datagen_blur(int sx, int sy, int sz, int ncomp, const float* src, float* dst, float* tmpA, float* tmpB, float sigma,
                    int* mdim_host, void* stream);

/* calcCenterOfMass.  Each term density * (i + 0.5f | j + 0.5f | k + 0.5f) is one fp32 product; the four sums (three moments and the
 * density itself) are taken in fp64 in a fixed order (per-thread strided, wavefront shuffles, workgroup partials, one workgroup's
 * tail), so every run gives the same bits.  With w = float(sum of density) > 1e-6f each out_host[c] = float(moment_c / sum) (an fp64
 * quotient rounded once), otherwise float(moment_c).  Synchronises the stream: one read-back of three floats. */
int mf_datagen_center_of_mass(int sx, int sy, int sz, const float* density, float* out_host, void* stream);

/* projectImg + the byte conversion of writePpm into img (device, h * w * 3 bytes, rows in FILE order: row r is image row j = h-1-r):
 * w = sx (2-D) or sx + sz + sx (3-D), h = max(sx, sy, sz).  One thread per pixel marches its view's depth axis in the reference's
 * order: pixel (i, j) over k; in 3-D also pixel (sx + k, j) over i and pixel (sx + sz + i, k) over j.  shadeMode 1 composites lit
 * surfaces: the light of every cell, from getGradient, is first written to `light` (n floats of scratch, distinct from val; needs every
 * axis of extent > 1 to have 3 cells); every other value accumulates smoke and touches no scratch (light may be NULL).  Then each
 * component / float(1. / scale), clamped to [0, 1], byte = (unsigned char)(255. * v).  `views` is a mask of the views to draw (1 z,
 * 2 x, 4 y; 7 = all; a 2-D grid has the z view only): pixels of no drawn view are 0.  Asynchronous. */
int mf_datagen_project(int sx, int sy, int sz, const float* val, float* light, int shadeMode, float scale, int views, uint8_t* img,
                       void* stream);

/* LaplaceOp on the interior: l = float(g(i+1) - 2.0 g + g(i-1)); l = float(l + (g(j+1) - 2.0 g + g(j-1))); in 3-D once more for k
 * (each parenthesis in double).  Border cells of lap keep their values; lap must not alias grid. */
int mf_datagen_laplacian(int sx, int sy, int sz, const float* grid, float* lap, void* stream);

/* CurvatureOp on the interior, expression by expression as commonkernels.h:83-101 (DESIGN.md has the map); the final division is by
 * the fp64 pow(max(denom, 1e-6f), 1.5).  Border cells of curv keep their values; curv must not alias grid. */
int mf_datagen_curvature(int sx, int sy, int sz, const float* grid, float* curv, float h, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MANTA_HIP_DATAGEN_H */
