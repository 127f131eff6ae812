/*
 * pggan_hip_augment.h — C-ABI of the differentiable augmentation of everything D sees (csrc/augment.hip): a gather with its exact
 * transpose, the kernel that turns uniform draws into the per-image parameter table, and the sign count of the adaptive controller.
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding
 * parses this header into tables of its own (_lib.AUGMENT_SIGNATURES / AUGMENT_CONSTANTS); the wrappers are ops.augment_apply /
 * augment_adjoint / augment_table / score_signs, the public face is augment.Augmenter.
 *
 * Definition (restated for the CPU in augment.py's numpy twin and, as a loop nest, in tests/augment_ref.py).
 *   images   fp32 [N][C][H][W], H and W powers of two in 4 .. PG_AUGMENT_MAX_SIZE;
 *   table    int32 [N][PG_AUGMENT_COLS], one row per image: (flags, dy, dx, y0, y1, x0, x1, gain_bits).  flags bit 0
 *            (PG_AUGMENT_FLIP): the x-flip; bit 1 (PG_AUGMENT_GAIN): the gain applies; gain_bits: the fp32 gain b, its bits as int32.
 *   forward  y[n][c][i][j] = +0.0 if y0 <= i < y1 and x0 <= j < x1 (the cutout); otherwise with j' = flip ? W - 1 - j : j and the source
 *            pixel (i - dy, j' - dx): +0.0 if that lies outside the image (zero padding), else x[n][c][i - dy][j' - dx] -- plus b (one
 *            fp32 add) where the row's gain flag is set and bit c of `channel_mask` is.  A row without gain copies bits (-0.0 stays
 *            -0.0, a NaN keeps its payload); the row (0, 0, 0, 0, 0, 0, 0, 0) copies the image.
 *   adjoint  gx[n][c][r][s] = gy[n][c][i][j] for the one (i, j) whose source is (r, s) -- i = r + dy, j' = s + dx, j = flip ? W - 1 - j'
 *            : j' -- where 0 <= i < H, 0 <= j' < W and (i, j) lies outside the cutout; +0.0 otherwise.  The gain has derivative 1.
 * Both are gathers: neither accumulates, neither uses atomics, both write every output element and give the same bits from run to run.
 * Any int32 is a valid table entry: a shift is clamped to the image's size and a cutout edge to the image (which changes nothing), and only
 * 16-byte words that lie inside the source plane are loaded.
 */
#ifndef PGGAN_HIP_AUGMENT_H
#define PGGAN_HIP_AUGMENT_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_AUGMENT_COLS 8
#define PG_AUGMENT_FLIP 1
#define PG_AUGMENT_GAIN 2
#define PG_AUGMENT_MAX_SIZE 4096
#define PG_AUGMENT_MAX_SCORES (1 << 20)

/* pg_augment_apply / pg_augment_adjoint: x (gy) and out (gx) [N][C][H][W] fp32, 16-byte aligned, not overlapping; table [N][8] int32,
 * 16-byte aligned.  A workgroup works on one plane; a thread owns four consecutive columns of one output row: it cuts them out of the one
 * or two aligned 16-byte words of the source row that hold them (a word lies wholly inside or wholly outside a row, W being a multiple of
 * 4; the load of a word outside is redirected to a word inside the plane and discarded: it counts as zeros, which IS the padding),
 * reverses them under a flip and stores 16 bytes.  `channel_mask`: bit c set = channel c takes the gain (pg_augment_apply only).
 * NULL pointer, N or C < 1, C > 32, H or W < 1, overlapping tensors: PG_E_ARG.  H or W not a power of two in 4 .. PG_AUGMENT_MAX_SIZE:
 * PG_E_UNSUP.  Misaligned base: PG_E_ALIGN. */
int pg_augment_apply(const float* x, const int* table, float* out, int64_t N, int C, int H, int W, int channel_mask, pg_stream_t stream);
int pg_augment_adjoint(const float* gy, const int* table, float* gx, int64_t N, int C, int H, int W, pg_stream_t stream);

/* pg_augment_table: U [rows][8] fp32 draws k / 2^24 of pg_uniform_f32 -> table [rows][8] int32; one thread per row.  Every operation of
 * a row is enabled when its own draw is below `p` (p = 0: the identity row; p = 1: every operation of the policy).  Columns of U:
 *   0  flip enable     1  flip coin (< 0.5); the bits below the coin, ug = 2 u1 - floor(2 u1), are the gain draw
 *   2  shift enable    3  dy draw       4  dx draw
 *   5  cutout enable   6  cutout centre: t = 4096 u6, uy = floor(t) / 4096, ux = t - floor(t) (12 bits each: exactly uniform over a
 *                         power of two <= 4096 positions)
 *   7  gain enable
 * All arithmetic is fp32 without contraction, every product is followed by its floor:
 *   flip    flags bit 0 = `flip` != 0 and u0 < p and u1 < 0.5
 *   shift   my = floor(ry H), dy = min(floor(u3 (2 my + 1)), 2 my) - my;  mx = floor(rx W), dx likewise from u4
 *   cutout  hc = floor(ch H + 0.5), wc = floor(cw W + 0.5); nothing if either is 0.  cy = floor(uy H), cx = floor(ux W);
 *           [y0, y1) = [max(cy - hc / 2, 0), min(cy - hc / 2 + hc, H)) (integer division), or [0, H) when hc >= H: ratio 1.0 on an axis
 *           masks that whole axis (a full-height time mask, a full-width frequency mask); [x0, x1) likewise
 *   gain    flags bit 1 = `gain` > 0 and u7 < p;  b = (2 ug - 1) gain  (2 ug - 1 is exact, one rounding)
 * A disabled operation leaves its columns 0.  NULL pointer, rows < 1, a ratio outside [0, 1], p outside [0, 1], gain < 0 (or any of them
 * NaN): PG_E_ARG.  H or W not a power of two in 4 .. PG_AUGMENT_MAX_SIZE: PG_E_UNSUP.  U or table not 16-byte aligned: PG_E_ALIGN. */
int pg_augment_table(const float* U, int64_t rows, int H, int W, float ry, float rx, float ch, float cw, float gain, int flip, float p,
                     int* table, pg_stream_t stream);

/* pg_score_signs: one workgroup.  acc [2] fp64 (8-byte aligned): acc[0] += sum_{i < n} sign(s[i]) with sign(+-0) = 0 (and sign(NaN) = 0),
 * acc[1] += n.  The sum is an integer formed in a fixed order, so both updates are exact up to 2^53.  1 <= n <= PG_AUGMENT_MAX_SCORES,
 * else PG_E_ARG;
 * acc not 8-byte aligned: PG_E_ALIGN. */
int pg_score_signs(const float* s, int64_t n, double* acc, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_AUGMENT_H */
