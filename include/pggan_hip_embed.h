/*
 * pggan_hip_embed.h — C-ABI of the random-embedding half of libpggan_hip.so (csrc/embed.hip): the ends of a randomly initialised
 * convolutional embedding of uint8 images (Naeem et al. 2020) and the fp64 moments of its features, for the Frechet distance `fd`.
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding
 * parses this header into tables of its own (_lib.EMBED_SIGNATURES / EMBED_CONSTANTS); the wrappers are ops.emb_stem_u8_bf16 /
 * emb_pool2_bf16 / emb_gap_f32 / fd_moments_f64.  The 3x3 layers between the ends are pg_smp_conv3_bf16 (include/pggan_hip_sampling.h).
 *
 * Definition (restated for the CPU in tests/fd_ref.py).  bf16 tensors are uint16_t bit patterns, rne(v) is the
 * round-to-nearest-even of an fp32 value to bf16 of the sampling path.  No atomics; every output element has one writer and a fixed
 * order of operations: the three ends equal their numpy float32 restatement bit for bit, and two calls of any entry point give the
 * same bits.  Nothing is allocated and nothing outside the tensors is read.
 */
#ifndef PGGAN_HIP_EMBED_H
#define PGGAN_HIP_EMBED_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Channels of the stem's output (the narrowest input pg_smp_conv3_bf16 takes) and the most image channels it reads. */
#define PG_EMB_STEM_CH 8
#define PG_EMB_MAX_C 4
/* pg_fd_moments_f64: rows of one slice, rows and columns of a workgroup's tile of cov, and the feature counts it takes. */
#define PG_FD_SLICE 256
#define PG_FD_TILE 64
#define PG_FD_MIN_F 16
#define PG_FD_MAX_F 512

/* pg_emb_stem_u8_bf16: x [M][C][H][W] uint8 -> y [M][H][W][PG_EMB_STEM_CH] bf16 (NHWC).  For c < C
 *                          y = rne((float(x) - 127.5f) / 127.5f)
 *                      one fp32 subtraction, one correctly rounded fp32 division, one rounding; channels C .. 7 are +0.  One 16-byte
 *                      store per pixel.  1 <= C <= PG_EMB_MAX_C (PG_E_ARG otherwise); 16-byte aligned bases (PG_E_ALIGN).  One launch.
 * pg_emb_pool2_bf16:   x [N][H][W][Ch] bf16 -> y [N][H/2][W/2][Ch] bf16, with a_uv = x[n][2 h + u][2 w + v][c] in fp32
 *                          y = rne(((a00 + a01) + (a10 + a11)) * 0.25f)
 *                      in exactly that order.  H and W even (PG_E_ARG), Ch % 8 == 0 and 16-byte aligned bases (PG_E_ALIGN).  One launch.
 * pg_emb_gap_f32:      x [N][H][W][Ch] bf16 -> f [N][Ch] fp32 = (sum over (h, w) in ascending row-major order, in fp32 from 0.0f)
 *                      * (1.0f / (float)(H W)): one rounding per addition, and the product is exact where H W is a power of two.
 *                      H W < 2^24 (PG_E_UNSUP); 16-byte aligned bases (PG_E_ALIGN).  One launch.
 * pg_fd_moments_f64:   x [M][F] fp32 -> mean [F], cov [F][F] fp64,
 *                          mean = sum_r x_r / M          cov = sum_r (x_r - mean)(x_r - mean)^T / (M - 1)
 *                      with the centring taken as (double)x - mean on the kernel's own mean.  M >= 2, F % 16 == 0 and
 *                      PG_FD_MIN_F <= F <= PG_FD_MAX_F (PG_E_ARG otherwise); M <= 2^31 (PG_E_UNSUP); x 16-byte, the rest 8-byte
 *                      aligned (PG_E_ALIGN).
 *                      The rows are cut into S = ceil(M / PG_FD_SLICE) slices (the cut depends on M alone) and the columns into
 *                      B = ceil(F / PG_FD_TILE) blocks; T = B (B + 1) / 2 tiles of cov lie on or above the diagonal.  `scratch` holds
 *                      scratch_doubles >= S (F + T PG_FD_TILE PG_FD_TILE) fp64 values (fewer: PG_E_ARG); the call writes every one
 *                      of the first that many.  Four launches:
 *                        1. column sums of every slice in fp64: four runs of 64 rows in ascending row order, combined in ascending
 *                           run order;
 *                        2. mean = (the slices' sums added in ascending slice order) / M;
 *                        3. one workgroup per (slice, tile): the centred operands of 32 rows at a time are staged through LDS in
 *                           fp64 -- rows at or past M and columns at or past F as exact zeros AFTER the centring -- and accumulated
 *                           on v_mfma_f64_16x16x4_f64, four rows per instruction in ascending row order; the tile's partial goes
 *                           to scratch;
 *                        4. cov[i][j] = cov[j][i] = (the slices' partials of element (i, j), i <= j, added in ascending slice
 *                           order) / (M - 1): computed on or above the diagonal only and mirrored, so cov == cov^T bit for bit. */
int pg_emb_stem_u8_bf16(const uint8_t* x, uint16_t* y, int64_t M, int C, int H, int W, pg_stream_t stream);
int pg_emb_pool2_bf16(const uint16_t* x, uint16_t* y, int64_t N, int H, int W, int Ch, pg_stream_t stream);
int pg_emb_gap_f32(const uint16_t* x, float* f, int64_t N, int H, int W, int Ch, pg_stream_t stream);
int pg_fd_moments_f64(const float* x, int64_t M, int F, double* mean, double* cov, double* scratch, int64_t scratch_doubles,
                      pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_EMBED_H */
