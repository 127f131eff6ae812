/*
 * pggan_hip_projection.h — C-ABI of the latent projection's image loss (csrc/projection.hip): the multi-resolution ("pyramid") squared
 * error between two image batches and its gradient with respect to the first.  It is the objective of projection.Projector, which
 * searches the latent whose generated image matches a given one ("Latent projection").
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding
 * parses this header into tables of its own (_lib.PROJECTION_SIGNATURES / PROJECTION_CONSTANTS); the wrapper is ops.pyramid_loss.
 *
 * The definition (restated in float64 for the CPU in tests/projection_ref.py).  Per sample n, images NCHW fp32 [N][C][r][r], r a power
 * of two in 4 .. PG_PYR_MAX_SIDE, 1 <= C <= PG_PYR_MAX_C:
 *   e      = img - target
 *   P_l(e) = the l-fold 2x2 box mean of e, side r_l = r >> l;  l = 0 .. log2(r / 4): the coarsest level is 4x4, r = 4 has one level
 *   loss[n]       = sum_l  w_l * mean_{c,y,x} P_l(e)[n]^2
 *   grad[n,c,y,x] = sum_l  w_l * 2 / (C r_l^2) * 4^-l * P_l(e)[n, c, y >> l, x >> l]          ( = d loss[n] / d img[n,c,y,x] )
 * The contract: e, every box mean, every sum of squares and both sums over l are fp64 in a fixed order; each output is rounded to fp32
 * once.  No atomics: two calls give the same bits.  img == target gives loss and grad exactly 0.  A level with w_l = 0 is skipped, not
 * multiplied: the result equals that of the pyramid without it bit for bit.  img and target are read once (loss only; every r <= 256)
 * or twice (r >= 512 with grad: the levels whose cells are larger than a workgroup's tile need every tile's mean first); grad is
 * written once.  Nothing is allocated: the caller passes the fp64 scratch.
 */
#ifndef PGGAN_HIP_PROJECTION_H
#define PGGAN_HIP_PROJECTION_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the level-0 tile of one workgroup is min(r, PG_PYR_TILE) pixels on a side */
#define PG_PYR_TILE 64
#define PG_PYR_MAX_SIDE 1024
#define PG_PYR_MAX_C 4
/* log2(PG_PYR_MAX_SIDE / 4) + 1 */
#define PG_PYR_MAX_LEVELS 9
/* fp64 words of scratch per (image plane, tile): 7 sums of squares, the tile mean, the cells of the levels above the tile */
#define PG_PYR_SCRATCH_PER_TILE 9

/* pg_pyr_loss_grad: img, target [N][C][r][r] fp32 (device) -> loss [N] fp32, grad [N][C][r][r] fp32 (NULL: the loss only, nothing else
 *                   is written).  weights: nlevels fp32 values ON THE HOST, read before the call returns, w_l of levels 0 .. nlevels - 1
 *                   (levels from nlevels up get 0); NULL with nlevels = 0 means every level with weight 1.  scratch: at least
 *                   8 * PG_PYR_SCRATCH_PER_TILE * N * C * tiles bytes on the device, tiles = (r / min(r, PG_PYR_TILE))^2; its contents
 *                   before the call do not matter and mean nothing after it.  grad must not overlap img, target or scratch.
 *                   PG_E_ARG: a null pointer, N < 1, C < 1, r < 4 or not a power of two, nlevels outside 0 .. log2(r / 4) + 1 (or 0
 *                   with weights, or > 0 without), a negative or non-finite weight, too little scratch.  PG_E_ALIGN: a base not 16-byte
 *                   aligned.  PG_E_UNSUP: r > PG_PYR_MAX_SIDE, C > PG_PYR_MAX_C, 2^31 or more (plane, tile) pairs.
 *                   Two launches (r <= 256 or loss only) or three.                                                                 */
int pg_pyr_loss_grad(const float* img, const float* target, const float* weights, int nlevels, float* grad, float* loss,
                     double* scratch, size_t scratch_bytes, int N, int C, int r, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_PROJECTION_H */
