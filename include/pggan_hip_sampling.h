/*
 * pggan_hip_sampling.h — C-ABI of the bf16 sampling path of libpggan_hip.so (csrc/sampling.hip): a forward-only evaluation of the
 * generator on the bf16 matrix cores, for everything that only LOOKS at G (sample grids, sound savers, the metric monitors).  The
 * training step stays fp32; nothing here has a backward pass.
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding
 * parses this header into tables of its own (_lib.SAMPLING_SIGNATURES / SAMPLING_CONSTANTS); the wrappers are in sampling.py.
 *
 * The contract (restated for the CPU in tests/sampling_ref.py).  rne(v) is round-to-nearest-even of an fp32
 * value to bf16 (NaN stays NaN); bf16 tensors are uint16_t bit patterns.  The rounding points, and there are no others:
 *   weights   wb = rne(w) of every 3x3 weight in its stored layout [3][3][Cout][Cin]; the equalized-lr constant c is NOT folded in,
 *             biases and the toRGB weights stay fp32.
 *   3x3 layer y = rne( PN( lrelu( c * sum_k a_k wb_k + b ) ) ),  a the bf16 input (nearest x2 upsampling evaluated in the gather),
 *             the products and the sum in fp32 on the MFMA, the epilogue in fp32, PN(v) = v / sqrt(mean_c v^2 + eps) skipped where
 *             the layer has none: ONE rounding, after PixelNorm.  Where the workgroup tile cannot hold every cout of a pixel the
 *             un-normalised fp32 value goes to a scratch tensor (PG_SMP_OUT_F32) and pg_smp_pixelnorm_bf16 normalises and rounds.
 *   toRGB     reads bf16 activations, computes in fp32 with fp32 weights, writes the fp32 NCHW image.
 * No atomics; every output element has one writer and a fixed summation order: two calls give the same bits.  Nothing is allocated.
 */
#ifndef PGGAN_HIP_SAMPLING_H
#define PGGAN_HIP_SAMPLING_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of pg_smp_conv3_bf16 */
#define PG_SMP_UPSAMPLE 1
#define PG_SMP_PIXELNORM 2
#define PG_SMP_OUT_F32 4
/* the widest layer whose PixelNorm pg_smp_conv3_bf16 fuses: every cout of a pixel in one wave's accumulators */
#define PG_SMP_PIXELNORM_MAX_COUT 128
/* the most image channels pg_smp_torgb_bf16 takes */
#define PG_SMP_TORGB_MAX_C 4

/* pg_smp_cast_bf16:      x [n] fp32 -> y [n] bf16 = rne(x).  One launch.
 * pg_smp_conv3_bf16:     x [N][Hin][Win][Cin] bf16, w [3][3][Cout][Cin] bf16, bias [Cout] fp32 (may be NULL) -> y [N][H][W][Cout], bf16
 *                        or (PG_SMP_OUT_F32) fp32, by the layer formula above: 3x3, pad 1, (H, W) = (Hin, Win), or twice that with
 *                        PG_SMP_UPSAMPLE (the input pixel of output position (h, w) is (h >> 1, w >> 1)).  H and W powers of two
 *                        >= 4 (PG_E_UNSUP otherwise); Cin % 8 == 0 and Cout % 8 == 0 (PG_E_ALIGN otherwise); fewer than 2^31
 *                        elements per tensor (PG_E_UNSUP).  PG_SMP_PIXELNORM needs Cout <= PG_SMP_PIXELNORM_MAX_COUT (PG_E_UNSUP:
 *                        ask for PG_SMP_OUT_F32 without it and run pg_smp_pixelnorm_bf16).  Implicit GEMM on
 *                        v_mfma_f32_16x16x32_bf16: a workgroup takes 64 .. 512 output pixels x up to 128 couts, a wave a quarter of
 *                        the pixels x those couts; K = (tap, cin) runs in ascending order in 32-channel chunks.  One launch.
 * pg_smp_pixelnorm_bf16: x [P][C] fp32 -> y [P][C] bf16 = rne(x / sqrt(mean_c x^2 + eps)).  C % 4 == 0 (PG_E_ALIGN).  One launch.
 * pg_smp_torgb_bf16:     x [N][H][W][Cin] bf16, w [C][Cin] fp32, bias [C] fp32 -> img [N][C][H][W] fp32
 *                          img = out_mul * (scale * sum_ci w x + bias)  +  prev_mul * (pscale * sum_ci pw px + pbias)
 *                        the second term only with px != NULL: px [N][H/2][W/2][PCin] bf16 read at (h >> 1, w >> 1), pw [C][PCin],
 *                        pbias [C] (reference network.py:131-138).  1 <= C <= PG_SMP_TORGB_MAX_C (PG_E_UNSUP otherwise), Cin % 8 == 0
 *                        and PCin % 8 == 0 (PG_E_ALIGN), H and W even with px.  One launch.                                    */
int pg_smp_cast_bf16(const float* x, uint16_t* y, int64_t n, pg_stream_t stream);
int pg_smp_conv3_bf16(const uint16_t* x, const uint16_t* w, const float* bias, void* y, int N, int Hin, int Win, int Cin, int Cout,
                      int flags, float scale, float slope, float eps, pg_stream_t stream);
int pg_smp_pixelnorm_bf16(const float* x, uint16_t* y, int64_t P, int C, float eps, pg_stream_t stream);
int pg_smp_torgb_bf16(const uint16_t* x, const float* w, const float* bias, float scale, float out_mul,
                      const uint16_t* px, const float* pw, const float* pbias, float pscale, float prev_mul, int PCin,
                      float* img, int N, int C, int H, int W, int Cin, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_SAMPLING_H */
