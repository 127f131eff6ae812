/*
 * pggan_hip_phase.h — C-ABI of the magnitude + instantaneous-frequency sound ends of libpggan_hip.so (csrc/phase.hip) and of the
 * two-channel real batch that trains on their images (csrc/real_batch.hip).  After Engel et al. 2019, "GANSynth": a generator that
 * produces log-magnitude plus instantaneous frequency (IF, the time derivative of the unwrapped phase) gives phase-coherent audio
 * with ONE inverse STFT, where a magnitude image needs Griffin-Lim's rounds and never recovers the phase.
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding
 * parses this header into tables of its own (_lib.PHASE_SIGNATURES / PHASE_CONSTANTS); the wrappers are in phase.py.
 *
 * Definitions (restated for the CPU in tests/magif_ref.py).  All fp64 without contraction, no atomics, every
 * output element has one writer and a fixed order of operations: the same bits from run to run.  Nothing is allocated.
 *   STFT      periodic Hann window, centred frames with reflect padding by n_fft/2, frame t at t hop (as pg_gl_pieces_f64);
 *             inverse: irfft x window x 2/3, overlap-add in ascending t (pg_overlap_add_f64), the padding cut off.
 *   analysis  S = STFT of the fp32 samples widened to fp64;  logmag = log1p(|S|);  phi = atan2(Im S, Re S) / pi with phi = 0 where
 *             |S| == 0 and phi[k][-1] = 0;  ifreq[k][t] = wrap(phi[k][t] - phi[k][t-1]),  wrap(d) = d - 2 floor(d/2 + 1/2) in [-1, 1).
 *             The first column is the phase itself; a running sum of a row gives the phase back modulo 2, in units of pi.
 *   image     channel 0 = clip(rint((logmag - lo) / (hi - lo) * 255), 0, 255);  channel 1 = rint((ifreq + 1) * 128) mod 256, round
 *             half to even: a circle of PG_PHASE_IF_LEVELS levels, level 0 is -pi and level PG_PHASE_IF_ZERO exactly 0.
 *   synthesis v = (img[0] - m_lo_in) m_scale + m_lo_out, mag = expm1(max(v, 0));  q = (img[1] - f_lo_in) f_scale + f_lo_out,
 *             ifreq = q / 128 - 1 (not clamped);  c[k][t] = sum_{s <= t} ifreq[k][s];  spec[k][t] = mag (cospi c, sinpi c) for k < H,
 *             0 for the bin H (Nyquist);  pieces = irfft(Hermitian extension of spec) x window x 2/3.
 */
#ifndef PGGAN_HIP_PHASE_H
#define PGGAN_HIP_PHASE_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n_fft is a power of two in PG_PHASE_MIN_N .. PG_PHASE_MAX_N (PG_E_UNSUP otherwise): image heights 4 .. 1024. */
#define PG_PHASE_MIN_N 8
#define PG_PHASE_MAX_N 2048
/* Levels of the IF circle of the uint8 image and the level of IF = 0. */
#define PG_PHASE_IF_LEVELS 256
#define PG_PHASE_IF_ZERO 128

/* pg_phase_analyse_f64:  y [batch][nsamp] fp32 mono -> logmag, ifreq [batch][bins][frames] fp64.  1 <= bins <= n_fft/2 + 1 and
 *                        1 <= frames <= 1 + nsamp / hop: only the bins and frames asked for are computed.  nsamp > n_fft/2 (the
 *                        reflect padding), hop >= 1, 1 <= batch <= 65535 (PG_E_ARG otherwise).  One workgroup per (frame, sample):
 *                        frames t and t - 1 are the real and the imaginary part of ONE complex radix-2 transform in LDS, separated
 *                        by the symmetry of a real signal's spectrum; the DC and Nyquist bins come out with an imaginary part of
 *                        exactly zero.  One launch.
 * pg_phase_quantise_u8:  logmag, ifreq [batch][plane] fp64 -> out [batch][2][plane] uint8 by the two image formulas, (lo, hi) the
 *                        magnitude range, hi > lo (PG_E_ARG otherwise).  One launch.
 * pg_phase_spectrum_f64: img [n][2][H][W] fp32 -> spec [n][W frames][H + 1 bins][2] fp64 (re, im): the two range changes, the clamp,
 *                        expm1, the running sum along W and sincospi.  H a power of two in 4 .. 1024 (PG_E_UNSUP otherwise), W <=
 *                        1024 (PG_E_ARG otherwise).  One workgroup per (bin, sample) scans its row of W values: thread i sums
 *                        ceil(W / 256) consecutive values, the 256 partial sums are scanned in LDS.  csum [n][H][W] fp64, which may
 *                        be NULL, receives the running sum c itself (the unreduced phase in units of pi).  One launch.
 * pg_phase_pieces_f64:   spec [batch][frames][n_fft/2 + 1][2] fp64 -> pieces [batch][frames][n_fft]: the Hermitian extension (the
 *                        imaginary parts of DC and Nyquist are ignored, as irfft does), the inverse transform, x window x 2/3 --
 *                        the summands of pg_overlap_add_f64.  frames x batch <= 2^22, batch <= 65535 (PG_E_ARG otherwise).  One
 *                        launch.                                                                                              */
int pg_phase_analyse_f64(const float* y, int64_t nsamp, int batch, double* logmag, double* ifreq, int n_fft, int hop, int bins,
                         int frames, pg_stream_t stream);
int pg_phase_quantise_u8(const double* logmag, const double* ifreq, uint8_t* out, int batch, int64_t plane, double lo, double hi,
                         pg_stream_t stream);
int pg_phase_spectrum_f64(const float* img, double* spec, double* csum, int n, int H, int W, double m_lo_in, double m_scale, double m_lo_out,
                          double f_lo_in, double f_scale, double f_lo_out, pg_stream_t stream);
int pg_phase_pieces_f64(const double* spec, double* pieces, int n_fft, int frames, int batch, pg_stream_t stream);

/* pg_real_batch_2ch_u8:  pg_real_batch_u8 (include/pggan_hip.h) for a stack of two-channel images, src [M][2][S][S]: the same
 *                        kernels, arguments, results and error codes, with C = 2 in place of its C in {1, 3}.                  */
int pg_real_batch_2ch_u8(const uint8_t* src, int64_t M, int S, int depthdiff, const int64_t* idx, const uint8_t* flip, int n,
                         float* out, double alpha, double min_in, double max_in, double min_out, double max_out, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_PHASE_H */
