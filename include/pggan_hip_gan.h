/*
 * pggan_hip_gan.h — C-ABI of the selectable GAN objectives of libpggan_hip.so (csrc/gan_losses.hip): the loss block of the
 * non-saturating logistic, hinge and least-squares objectives beside WGAN, and the tangent seed of the R1 penalty.
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding
 * parses this header into tables of its own (_lib.GAN_SIGNATURES / GAN_CONSTANTS); the wrappers are in ops.py (gan_d_loss, gan_g_loss,
 * r1_seed) and the public interface is gan_losses.py.
 *
 * Definition (restated in fp64 in tests/gan_losses_ref.py).  s_r[n], s_f[n]: D's scores on the real and on the
 * generated images, s[n] = D(G(z))[n] in the G step, n < N.
 *   d_cost = (1/N) sum_n (F[n] + R[n] + P[n]),   g_cost = (1/N) sum_n L[n],   gscore = d cost / d score (the 1/N included)
 *
 *   kind               R[n] (real)          F[n] (fake)          L[n] (generator)
 *   PG_GAN_WGAN        -s_r                 s_f                  -s
 *   PG_GAN_LOGISTIC    softplus(-s_r)       softplus(s_f)        softplus(-s)          (non-saturating)
 *   PG_GAN_HINGE       max(0, 1 - s_r)      max(0, 1 + s_f)      -s
 *   PG_GAN_LSGAN       (s_r - 1)^2          s_f^2                (s - 1)^2             (no factor 1/2)
 *
 *   every kind: R[n] += drift s_r^2 (derivative 2 drift s_r);
 *   softplus(x) = max(x, 0) + log1p(exp(-|x|)), its derivative 1 / (1 + e^-x) for x >= 0 and e^x / (1 + e^x) for x < 0: nothing
 *   overflows at |x| = 1e4;  the hinge derivative at the kink is 0: dR/ds_r = -1 iff s_r < 1, dF/ds_f = 1 iff s_f > -1;
 *   NaN scores are out of contract.
 */
#ifndef PGGAN_HIP_GAN_H
#define PGGAN_HIP_GAN_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_GAN_WGAN 0
#define PG_GAN_LOGISTIC 1
#define PG_GAN_HINGE 2
#define PG_GAN_LSGAN 3

/* pg_gan_d_loss: s [groups N] = [real(N) | fake(N) | (mixed(N))], groups 2 or 3;  pen [N] = P[n], or NULL for no penalty.
 *                d_real[n] = R[n], d_fake[n] = F[n], d_cost[0] as above; gscore [groups N]: dR/ds_r / N, dF/ds_f / N and, with three
 *                groups, zeros for the last third (the penalty reaches the weights through the tangent pass, not through the scores).
 *                One wavefront: lane l accumulates n = l, l + 64, ... in ascending order, then a fixed butterfly over the 64 lanes;
 *                no atomics, the same bits from call to call.  Every product, sum and quotient is one rounded fp32 operation as
 *                written in csrc/gan_losses.hip (no contraction).  kind outside PG_GAN_*, groups outside {2, 3}: PG_E_ARG.
 * pg_gan_g_loss: s [N] -> g_cost[0], gscore [N] = dL/ds / N.  Same reduction.
 * pg_r1_seed:    the R1 penalty (gamma / 2) |g[n]|^2 and its tangent seed:  g [N][E] the image gradient, ss [N] its row sums of squares
 *                (pg_row_sumsq) -> pen[n] = (0.5 gamma) ss[n], u [N][E] = (inv_n gamma) g, one product per element.  pg_gp_seed's launch
 *                geometry (one float4 per thread, 256 threads, at most 1024 workgroups per row, grid-stride beyond) over the N E
 *                elements as one range, plus a scalar tail of N E mod 4 elements: E need not be a multiple of 4.  g and u 16-byte
 *                aligned (PG_E_ALIGN otherwise).                                                                                  */
int pg_gan_d_loss(const float* s, const float* pen, float* d_cost, float* d_real, float* d_fake, float* gscore, int N, int groups,
                  int kind, float drift, pg_stream_t stream);
int pg_gan_g_loss(const float* s, float* g_cost, float* gscore, int N, int kind, pg_stream_t stream);
int pg_r1_seed(const float* g, const float* ss, float* pen, float* u, int N, int64_t E, float gamma, float inv_n, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_GAN_H */
