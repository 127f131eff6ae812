/*
 * pggan_hip_kid.h — C-ABI of the kernel-distance half of libpggan_hip.so (csrc/kid.hip): the tile sums of the cubic polynomial kernel
 * between two sets of feature vectors in fp64, for the unbiased MMD^2 estimator `kid` (Binkowski et al. 2018) over the features of the
 * random embedding (include/pggan_hip_embed.h).
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding parses this header into
 * tables of its own (_lib.KID_SIGNATURES / KID_CONSTANTS); the wrapper is ops.kid_tilesums_f64, the statistic metrics.kid_statistic.
 *
 * Definition (restated for the CPU in tests/kid_ref.py).  No atomics; every output element has one writer and a
 * fixed order of operations, so two calls give the same bits.  Nothing is allocated and nothing outside the tensors is read.
 */
#ifndef PGGAN_HIP_KID_H
#define PGGAN_HIP_KID_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pg_kid_tilesums_f64: rows and columns of x / y that one output sum covers, and the feature counts it takes. */
#define PG_KID_TILE 64
#define PG_KID_MIN_F 16
#define PG_KID_MAX_F 512

/* pg_kid_tilesums_f64: x [M][F], y [N][F] fp32 -> sums [A][B] fp64 with A = ceil(M / PG_KID_TILE), B = ceil(N / PG_KID_TILE); every
 *                      element is written:
 *                          sums[a][b] = sum of k(x_i, y_j) over i in row tile a with i < M and j in column tile b with j < N,
 *                                       without the pairs i == j when skip_diagonal
 *                          k = (t * t) * t          t = gamma * g + coef0          g = sum_f (double)x_if * (double)y_jf
 *                      t is one fp64 multiplication and one fp64 addition (not fused), k two fp64 multiplications.  g is accumulated
 *                      on v_mfma_f64_16x16x4_f64 from 0 in ascending f, four features per instruction; the products of two fp32
 *                      values are exact in fp64, so only the additions round.
 *                      Ragged tiles: rows at or past M and columns at or past N are never loaded; their operands are exact zeros and
 *                      their pairs are left out of the sum AFTER the kernel function is applied (a zero row has k = coef0^3, not 0).
 *                      The pairs left out (those, and i == j under skip_diagonal) enter the sums below as +0.0.
 *                      Self form: y == NULL means y = x and N = M.  Only the tiles a <= b are computed, and sums[b][a] = sums[a][b]
 *                      is mirrored bit for bit.  skip_diagonal is allowed in the self form only (PG_E_ARG otherwise).
 *                      Summation order of one tile (it depends on (M, N, F) alone): one workgroup of four waves per tile; wave
 *                      w = 2 wr + wc owns the 32 x 32 quarter (wr, wc) as 2 x 2 instruction tiles (p, q) of 16 x 16.  Lane l holds
 *                      element g = 0 .. 3 of tile (p, q): row 32 wr + 16 p + (l >> 4) + 4 g, column 32 wc + 16 q + (l & 15).
 *                        1. every lane adds its 16 values from 0.0 in the order p, q, g (g innermost);
 *                        2. the 64 lanes of a wave are combined by a butterfly, s <- s + s(lane ^ d) for d = 32, 16, 8, 4, 2, 1
 *                           (an addition is commutative, so every lane ends with the same bits);
 *                        3. sums[a][b] = ((w0 + w1) + w2) + w3 over the four waves' values.
 *                      That is 15 + 6 + 3 additions on the path of any one value; no sum has more than PG_KID_TILE^2 terms.
 *                      M, N >= 1, F % 16 == 0 and PG_KID_MIN_F <= F <= PG_KID_MAX_F (PG_E_ARG otherwise); at most 65535 row tiles
 *                      (PG_E_UNSUP); x and y 16-byte, sums 8-byte aligned (PG_E_ALIGN).  One launch. */
int pg_kid_tilesums_f64(const float* x, int64_t M, const float* y, int64_t N, int F, double gamma, double coef0, int skip_diagonal,
                        double* sums, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_KID_H */
